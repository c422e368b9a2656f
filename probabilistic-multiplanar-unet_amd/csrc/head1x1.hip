// OutConv 1x1 (+ sigmoid) head: forward, backward to the last layer's gradient (alone, fused with that
// layer's BatchNorm+ReLU backward partial sums and the head's own weight gradient, or applied as dz) and
// the weight / bias gradient (PMU/model/unet/unet_parts.py:70-76, unet_model.py:48-49).
// All reductions write per-block partial slabs that are summed in a fixed order (fp64).
#include <type_traits>

#include "pmu_stage.h"

// ---- channel-quad x pixel-group fast paths of the 1x1 head (single unpooled BN+ReLU source,
// C = 4*CQ with CQ a power of two <= 64): a wave reads CQ consecutive quads of 64/CQ pixels, i.e.
// contiguous runs of NHWC rows, instead of one strided row per thread.  The pixel index is decoded in
// 32 bits (P < 2^31).
static bool head_fast_shape(int C, long long P) {
  const int CQ = C >> 2;
  return (C & 3) == 0 && CQ <= 64 && (CQ & (CQ - 1)) == 0 && P < (1LL << 31);
}
static bool host_head_fast(const pmu_frame* in) {
  const pmu_src& s = in->src[0];
  return in->nsrc == 1 && s.mode == PMU_SRC_BNRELU && s.pool == PMU_POOL_NONE && s.off_h == 0 && s.off_w == 0 &&
         s.H == in->H && s.W == in->W && head_fast_shape(s.C, (long long)in->N * in->H * in->W);
}

constexpr int HPPB = 2048;  // pixels per block in the fast head kernels

// ---------------- forward ----------------
namespace {
__global__ __launch_bounds__(256) void head_fwd_kernel(DevFrame f, const float* __restrict__ w, const float* __restrict__ b,
                                                       int K, int do_sigmoid, float* __restrict__ y) {
  const long long HW = (long long)f.H * f.W;
  const long long P = (long long)f.N * HW;
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int ww = (int)(p % f.W), hh = (int)((p / f.W) % f.H), n = (int)(p / HW);
  float acc[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) acc[k] = (k < K && b) ? b[k] : 0.f;
  for (int c = 0; c < f.C; c += 4) {
    const float4 v = frame_value4(f, n, hh, ww, c);
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e >= f.C) break;
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k)
        if (k < K) acc[k] = fmaf(vv[e], w[k * f.C + c + e], acc[k]);
    }
  }
  const long long pix = p - (long long)n * HW;
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) {
    if (k >= K) break;
    float v = acc[k];
    if (do_sigmoid) v = 1.f / (1.f + expf(-v));
    y[((long long)n * K + k) * HW + pix] = v;
  }
}

// 1x1 head forward on one unpooled BN+ReLU source: thread = (channel quad cq, pixel group), the 16 B
// loads of a pixel's quads coalesce into its whole C-channel row; per class the quad dot products
// are summed over the pixel's CQ lanes by xor shuffles and lane cq == 0 writes y[n][k][pix].
// (One thread per pixel read a 16-B piece of 64 different rows per load instruction.)
// XBF: the source's x in bf16 (a compile-time choice: a load under the storage-type branch would be
// waited for on its own).  HU pixels per thread per round, their loads issued together (address
// clamped to the block's last pixel, only the stores predicated): one pixel per round left a global
// round trip exposed per pixel for one class (c2: 0.19 -> 0.14 ms); with three classes the batch of
// four measured slower (c5: 0.31 -> 0.37 ms; with the DPP class sums 0.32 vs 0.26), so HU = 1 there.
// The per-class sum over a pixel's CQ lanes is pmu_group_sum: DPP moves instead of xor shuffles (one
// ds_bpermute round trip per step): c5 0.286 -> 0.260 ms, c2 0.142 -> 0.138 ms, bit-identical
template <bool XBF, int HU>
__global__ __launch_bounds__(256) void head_fwd_fast_kernel(DevFrame f, const float* __restrict__ w,
                                                            const float* __restrict__ b, int K, int do_sigmoid,
                                                            float* __restrict__ y) {
  const int tid = threadIdx.x;
  const int C = f.C, CQ = C >> 2, PG = 256 / CQ;
  const int cq = tid & (CQ - 1), pg = tid / CQ;
  const unsigned HWu = (unsigned)f.H * (unsigned)f.W;
  const long long P = (long long)f.N * HWu;
  const float4 sc = *reinterpret_cast<const float4*>(f.s0.coef + 4 * cq);
  const float4 sh = *reinterpret_cast<const float4*>(f.s0.coef + C + 4 * cq);
  float4 wq[HEAD_KMAX];
  float bk[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) {
    wq[k] = k < K ? *reinterpret_cast<const float4*>(w + k * C + 4 * cq) : make_float4(0.f, 0.f, 0.f, 0.f);
    bk[k] = (k < K && b) ? b[k] : 0.f;
  }
  const unsigned pend = (unsigned)min(P, (long long)(blockIdx.x + 1) * HPPB);
  // a round's loads; with HU > 1 the next round's are issued before this round's stores (waiting for
  // them then does not wait, in-order vmcnt, for those stores: c2 138 -> 134 us); with HU = 1 that
  // measured slower (c5 260 -> 349 us), so a round loads its own pixel there
  auto load_round = [&](unsigned q0, float4 (&zo)[HU]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const unsigned p = min(q0 + u * PG, pend - 1);
      const long long i = (long long)p * C + 4 * cq;
      zo[u] = XBF ? pmu_ld4(reinterpret_cast<const unsigned short*>(f.s0.x) + i) : pmu_ld4(f.s0.x + i);
    }
  };
  float4 zx[HU], zn[HU];
  const unsigned pfirst = blockIdx.x * HPPB + pg;
  if (HU > 1 && pfirst < pend) load_round(pfirst, zx);
  for (unsigned p0 = pfirst; p0 < pend; p0 += HU * PG) {  // 32-bit decode (P < 2^31)
    if constexpr (HU > 1) {
      if (p0 + HU * PG < pend) load_round(p0 + HU * PG, zn);
    } else {
      load_round(p0, zx);
    }
#pragma unroll
    for (int u = 0; u < HU; ++u) {
      const unsigned p = p0 + u * PG;
      const float4 a = pmu_bnrelu4(zx[u], sc, sh);
      const unsigned pc = min(p, pend - 1);
      const unsigned n = pc / HWu, pix = pc - n * HWu;
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k) {
        if (k >= K) break;
        float v = fmaf(a.x, wq[k].x, fmaf(a.y, wq[k].y, fmaf(a.z, wq[k].z, a.w * wq[k].w)));
        v = pmu_group_sum(v, CQ);  // (bit-identical to the xor-shuffle butterfly it replaces)
        v += bk[k];
        if (do_sigmoid) v = 1.f / (1.f + expf(-v));
        if (cq == 0 && p < pend) y[(size_t)(n * K + k) * HWu + pix] = v;
      }
    }
    if constexpr (HU > 1) {
#pragma unroll
      for (int u = 0; u < HU; ++u) zx[u] = zn[u];
    }
  }
}
}  // namespace

extern "C" int pmu_head1x1_fwd(const pmu_frame* in, const float* w, const float* b, int K, int do_sigmoid,
                               float* y, void* stream) {
  PMU_REQUIRE(valid_frame(in, true) && w && y && K >= 1 && K <= HEAD_KMAX);
  const DevFrame f = make_dev_frame(in);
  const long long P = (long long)in->N * in->H * in->W;
  if (host_head_fast(in)) {
    hipLaunchKernelGGL(f.s0.xbf ? (K == 1 ? head_fwd_fast_kernel<true, 4> : head_fwd_fast_kernel<true, 1>)
                                : (K == 1 ? head_fwd_fast_kernel<false, 4> : head_fwd_fast_kernel<false, 1>),
                       dim3((unsigned)pmu_cdiv(P, HPPB)), dim3(256), 0, (hipStream_t)stream,
                       f, w, b, K, do_sigmoid, y);
    PMU_CHECK_LAUNCH();
    return PMU_OK;
  }
  hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)pmu_cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream,
                     f, w, b, K, do_sigmoid, y);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// ---------------- backward: dl = dy * sigmoid', da = dl w ----------------
namespace {
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                       int do_sigmoid, const float* __restrict__ w, int K, int C,
                                                       int N, int H, int W, float* __restrict__ dl, float* __restrict__ da) {
  const long long HW = (long long)H * W;
  const long long P = (long long)N * HW;
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int n = (int)(p / HW);
  const long long pix = p - (long long)n * HW;
  float g[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) {
    g[k] = 0.f;
    if (k < K) {
      const long long i = ((long long)n * K + k) * HW + pix;
      float v = dy[i];
      if (do_sigmoid) { const float s = y[i]; v = v * (s * (1.f - s)); }
      g[k] = v;
      dl[i] = v;
    }
  }
  for (int c = 0; c < C; c += 4) {
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = 0.f;
      if (c + e < C) {
#pragma unroll
        for (int k = 0; k < HEAD_KMAX; ++k)
          if (k < K) s = fmaf(g[k], w[k * C + c + e], s);
      }
      o[e] = s;
    }
    if (c + 3 < C && (C % 4) == 0) {
      *reinterpret_cast<float4*>(da + p * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int e = 0; e < 4 && c + e < C; ++e) da[p * C + c + e] = o[e];
    }
  }
}

// BNR: also the BatchNorm+ReLU backward partial sums of the layer feeding the head (da is its
// gradient): part[block][2][C] = (sum g, sum g*xhat), g = da * (z*scale+shift > 0),
// xhat = (z-mean)*invstd — what bn_bwd_reduce would read da and z again for
// WG (with BNR): also the head's weight / bias gradient partials ws[block][K][C+1] from the same z
// reads, a = relu(z*scale+shift) — wgrad1x1_fast_kernel's block, thread mapping and summation order, so
// rows_sum_split4_kernel turns them into the same dw, db; dl is then not written
struct HeadBnr {
  const float* z;
  const float* coef;
  const float* mean;
  const float* invstd;
  float* part;
  float* ws;
};

template <bool BNR, bool WG = false>
__global__ __launch_bounds__(256) void head_bwd_fast_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                            int do_sigmoid, const float* __restrict__ w, int K, int C,
                                                            long long HW, long long P, float* __restrict__ dl,
                                                            float* __restrict__ da, HeadBnr bn) {
  __shared__ float red[BNR ? 4 * 2 * 256 : 1];
  __shared__ float redw[WG ? 4 * HEAD_KMAX * 260 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CQ = C >> 2, PG = 256 / CQ;
  const int cq = tid & (CQ - 1), pg = tid / CQ;
  float4 wq[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k)
    wq[k] = k < K ? *reinterpret_cast<const float4*>(w + k * C + 4 * cq) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 sc, sh, mu, is;
  float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  float4 wacc[HEAD_KMAX];
  float waccb[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) { wacc[k] = make_float4(0.f, 0.f, 0.f, 0.f); waccb[k] = 0.f; }
  if (BNR) {
    sc = *reinterpret_cast<const float4*>(bn.coef + 4 * cq);
    sh = *reinterpret_cast<const float4*>(bn.coef + C + 4 * cq);
    mu = *reinterpret_cast<const float4*>(bn.mean + 4 * cq);
    is = *reinterpret_cast<const float4*>(bn.invstd + 4 * cq);
  }
  // 32-bit pixel decode (P < 2^31, host-checked): 64-bit divisions per pixel dominated
  const unsigned HWu = (unsigned)HW, pend = (unsigned)min(P, (long long)(blockIdx.x + 1) * HPPB);
  for (unsigned p = blockIdx.x * HPPB + pg; p < pend; p += PG) {
    const unsigned n = p / HWu, pix = p - n * HWu;
    float4 zz;
    if (BNR) zz = *reinterpret_cast<const float4*>(bn.z + (size_t)p * C + 4 * cq);  // in flight with dy
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 av;
    if (WG) av = pmu_bnrelu4(zz, sc, sh);
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) {
      if (k >= K) break;
      const size_t i = (size_t)(n * K + k) * HWu + pix;
      float g = dy[i];
      if (do_sigmoid) { const float sg = y[i]; g = g * (sg * (1.f - sg)); }
      if (!WG && cq == 0) dl[i] = g;
      o.x = fmaf(g, wq[k].x, o.x); o.y = fmaf(g, wq[k].y, o.y);
      o.z = fmaf(g, wq[k].z, o.z); o.w = fmaf(g, wq[k].w, o.w);
      if (WG) {
        wacc[k].x = fmaf(g, av.x, wacc[k].x); wacc[k].y = fmaf(g, av.y, wacc[k].y);
        wacc[k].z = fmaf(g, av.z, wacc[k].z); wacc[k].w = fmaf(g, av.w, wacc[k].w);
        waccb[k] += g;
      }
    }
    *reinterpret_cast<float4*>(da + (size_t)p * C + 4 * cq) = o;
    if (BNR) {
      const float ov[4] = {o.x, o.y, o.z, o.w}, zv[4] = {zz.x, zz.y, zz.z, zz.w};
      const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
      const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = fmaf(zv[e], scv[e], shv[e]) > 0.f ? ov[e] : 0.f;
        s1[e] += g;
        s2[e] = fmaf(g, (zv[e] - muv[e]) * isv[e], s2[e]);
      }
    }
  }
  if (BNR) {  // the wave's pixel groups by xor shuffles, then the 4 waves in order
#pragma unroll
    for (int e = 0; e < 4; ++e)
      for (int o = CQ; o < 64; o <<= 1) {
        s1[e] += __shfl_xor(s1[e], o, 64);
        s2[e] += __shfl_xor(s2[e], o, 64);
      }
    if (lane < CQ) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        red[(wave * 2 + 0) * 256 + 4 * cq + e] = s1[e];
        red[(wave * 2 + 1) * 256 + 4 * cq + e] = s2[e];
      }
    }
    __syncthreads();
    for (int o = tid; o < 2 * C; o += 256) {
      const int r = o / C, c = o - r * C;
      float t = 0.f;
      for (int wv = 0; wv < 4; ++wv) t += red[(wv * 2 + r) * 256 + c];
      bn.part[(long long)blockIdx.x * 2 * C + o] = t;
    }
  }
  if (WG) {  // as wgrad1x1_fast_kernel
    const int CW = C + 1;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) {
      if (k >= K) break;
      float v[5] = {wacc[k].x, wacc[k].y, wacc[k].z, wacc[k].w, waccb[k]};
#pragma unroll
      for (int e = 0; e < 5; ++e)
        for (int o = CQ; o < 64; o <<= 1) v[e] += __shfl_xor(v[e], o, 64);
      if (lane < CQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e) redw[(wave * HEAD_KMAX + k) * 260 + 4 * cq + e] = v[e];
        if (cq == 0) redw[(wave * HEAD_KMAX + k) * 260 + C] = v[4];
      }
    }
    __syncthreads();
    for (int o = tid; o < K * CW; o += 256) {
      const int k = o / CW, c = o - k * CW;
      float t = 0.f;
      for (int wv = 0; wv < 4; ++wv) t += redw[(wv * HEAD_KMAX + k) * 260 + c];
      bn.ws[(long long)blockIdx.x * K * CW + o] = t;
    }
  }
}
}  // namespace

extern "C" int pmu_head1x1_bwd(const float* dy, const float* y, int do_sigmoid, const float* w, int K, int C,
                               int N, int H, int W, float* dl, float* da, void* stream) {
  PMU_REQUIRE(dy && w && dl && da && K >= 1 && K <= HEAD_KMAX && C > 0 && (!do_sigmoid || y));
  const long long P = (long long)N * H * W;
  if (head_fast_shape(C, P)) {
    const HeadBnr nob{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(head_bwd_fast_kernel<false>, dim3((unsigned)pmu_cdiv(P, HPPB)), dim3(256), 0,
                       (hipStream_t)stream, dy, y, do_sigmoid, w, K, C, (long long)H * W, P, dl, da, nob);
    PMU_CHECK_LAUNCH();
    return PMU_OK;
  }
  hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)pmu_cdiv(P, 256)), dim3(256), 0, (hipStream_t)stream,
                     dy, y, do_sigmoid, w, K, C, N, H, W, dl, da);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// ---------------- backward fused with the BN+ReLU backward sums and the weight gradient ----------------
// f(integral_constant<int, K>, bool_constant<a>, bool_constant<b>) for the runtime class count K in
// 1..HEAD_KMAX and two runtime flags: the compile-time <KT, bool, bool> of the kernels below.  False if
// K is out of range (f not called).
template <int KV = 1, class F>
static bool head_dispatch(int K, bool a, bool b, F&& f) {
  if constexpr (KV <= HEAD_KMAX) {  // (the recursion ends at HEAD_KMAX + 1, which instantiates no f)
    if (K != KV) return head_dispatch<KV + 1>(K, a, b, f);
    const std::integral_constant<int, KV> kt;
    if (a && b) f(kt, std::true_type{}, std::true_type{});
    else if (a) f(kt, std::true_type{}, std::false_type{});
    else if (b) f(kt, std::false_type{}, std::true_type{});
    else f(kt, std::false_type{}, std::false_type{});
    return true;
  }
  return false;
}

namespace {
// The fused head backward (BNR + WG of head_bwd_fast_kernel) with KT classes and the sigmoid as
// compile-time constants and the pixel loop in batches of 4: every load of a batch (z, dy, y; clamped
// addresses, out-of-range pixels masked to 0) is issued before its da stores.  One pixel per
// iteration made each iteration's loads wait for the previous iteration's store (vmcnt counts loads
// and stores in order): 2.2 TB/s.  Same per-thread summation order as head_bwd_fast_kernel /
// wgrad1x1_fast_kernel (masked terms add exact zeros), so the results are bit-identical.
// STDA = false: da not stored (head_dz_kernel re-forms it for the last layer's dz, engine.HeadDa)
template <int KT, bool SIG, bool STDA = true>
__global__ __launch_bounds__(256) void head_bwd_fused_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                             const float* __restrict__ w, int C, long long HW,
                                                             long long P, float* __restrict__ da, HeadBnr bn) {
  // (no fp contraction: without the da store hipcc fused g = dy * y(1-y) into the bias sum's add, an
  // FMA where pmu_wgrad1x1 adds the rounded g — db then differed in the last bit)
#pragma clang fp contract(off)
  constexpr int B = 4;
  __shared__ float red[4 * 2 * 256];
  __shared__ float redw[4 * KT * 260];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CQ = C >> 2, PG = 256 / CQ;
  const int cq = tid & (CQ - 1), pg = tid / CQ;
  float4 wq[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) wq[k] = *reinterpret_cast<const float4*>(w + k * C + 4 * cq);
  const float4 sc = *reinterpret_cast<const float4*>(bn.coef + 4 * cq);
  const float4 sh = *reinterpret_cast<const float4*>(bn.coef + C + 4 * cq);
  const float4 mu = *reinterpret_cast<const float4*>(bn.mean + 4 * cq);
  const float4 is = *reinterpret_cast<const float4*>(bn.invstd + 4 * cq);
  const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
  const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w};
  float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  float4 wacc[KT];
  float waccb[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) { wacc[k] = make_float4(0.f, 0.f, 0.f, 0.f); waccb[k] = 0.f; }
  const unsigned HWu = (unsigned)HW, pend = (unsigned)min(P, (long long)(blockIdx.x + 1) * HPPB);
  for (unsigned p0 = blockIdx.x * HPPB + pg; p0 < pend; p0 += B * PG) {
    float4 zz[B];
    float g[B][KT];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const unsigned p = min(p0 + b * PG, pend - 1);
      const unsigned n = p / HWu, pix = p - n * HWu;
      zz[b] = *reinterpret_cast<const float4*>(bn.z + (size_t)p * C + 4 * cq);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const size_t i = (size_t)(n * KT + k) * HWu + pix;
        g[b][k] = dy[i];
        if (SIG) { const float sg = y[i]; g[b][k] = g[b][k] * (sg * (1.f - sg)); }
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const unsigned p = p0 + b * PG;
      const bool ok = p < pend;
      const float4 av = pmu_bnrelu4(zz[b], sc, sh);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const float gk = ok ? g[b][k] : 0.f;
        o.x = fmaf(gk, wq[k].x, o.x); o.y = fmaf(gk, wq[k].y, o.y);
        o.z = fmaf(gk, wq[k].z, o.z); o.w = fmaf(gk, wq[k].w, o.w);
        wacc[k].x = fmaf(gk, av.x, wacc[k].x); wacc[k].y = fmaf(gk, av.y, wacc[k].y);
        wacc[k].z = fmaf(gk, av.z, wacc[k].z); wacc[k].w = fmaf(gk, av.w, wacc[k].w);
        waccb[k] += gk;
      }
      const float ov[4] = {o.x, o.y, o.z, o.w}, zv[4] = {zz[b].x, zz[b].y, zz[b].z, zz[b].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = fmaf(zv[e], scv[e], shv[e]) > 0.f ? ov[e] : 0.f;
        s1[e] += gg;
        s2[e] = fmaf(gg, (zv[e] - muv[e]) * isv[e], s2[e]);
      }
      if (STDA && ok) *reinterpret_cast<float4*>(da + (size_t)p * C + 4 * cq) = o;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    for (int o = CQ; o < 64; o <<= 1) {
      s1[e] += __shfl_xor(s1[e], o, 64);
      s2[e] += __shfl_xor(s2[e], o, 64);
    }
  if (lane < CQ) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[(wave * 2 + 0) * 256 + 4 * cq + e] = s1[e];
      red[(wave * 2 + 1) * 256 + 4 * cq + e] = s2[e];
    }
  }
  const int CW = C + 1;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    float v[5] = {wacc[k].x, wacc[k].y, wacc[k].z, wacc[k].w, waccb[k]};
#pragma unroll
    for (int e = 0; e < 5; ++e)
      for (int o = CQ; o < 64; o <<= 1) v[e] += __shfl_xor(v[e], o, 64);
    if (lane < CQ) {
#pragma unroll
      for (int e = 0; e < 4; ++e) redw[(wave * KT + k) * 260 + 4 * cq + e] = v[e];
      if (cq == 0) redw[(wave * KT + k) * 260 + C] = v[4];
    }
  }
  __syncthreads();
  for (int o = tid; o < 2 * C; o += 256) {
    const int r = o / C, c = o - r * C;
    float t = 0.f;
    for (int wv = 0; wv < 4; ++wv) t += red[(wv * 2 + r) * 256 + c];
    bn.part[(long long)blockIdx.x * 2 * C + o] = t;
  }
  for (int o = tid; o < KT * CW; o += 256) {
    const int k = o / CW, c = o - k * CW;
    float t = 0.f;
    for (int wv = 0; wv < 4; ++wv) t += redw[(wv * KT + k) * 260 + c];
    bn.ws[(long long)blockIdx.x * KT * CW + o] = t;
  }
}

// The sum of the weight-gradient slabs (here and in pmu_wgrad1x1): out[o] = sum_r ws[r][o] for o < K*(C+1),
// split into dw[k][c] and db[k]; 64 outputs x 4 row phases
__global__ __launch_bounds__(1024) void rows_sum_split4_kernel(const float* __restrict__ ws, int R, int K, int C,
                                                               float* dw, float* db) {
  __shared__ double red[1024];
  const int CW = C + 1, Wd = K * CW;
  const int o = blockIdx.x * 64 + (threadIdx.x & 63);
  const double t = pmu_colsum64x16(ws, R, Wd, o, red);
  if (threadIdx.x < 64 && o < Wd) {
    const int k = o / CW, c = o - k * CW;
    if (c < C) dw[k * C + c] = (float)t;
    else if (db) db[k] = (float)t;
  }
}
}  // namespace

extern "C" int pmu_head1x1_bwd_bnr_ok(int N, int H, int W, int C) { return head_fast_shape(C, (long long)N * H * W); }

extern "C" int pmu_head1x1_bwd_tiles(int N, int H, int W) { return (int)pmu_cdiv((long long)N * H * W, HPPB); }

extern "C" int pmu_head1x1_bwd_bnr(const float* dy, const float* y, int do_sigmoid, const float* w, int K, int C,
                                   int N, int H, int W, float* dl, float* da, const float* z, const float* coef,
                                   const float* mean, const float* invstd, float* part, float* dw, float* db,
                                   float* ws, size_t ws_bytes, void* stream) {
  PMU_REQUIRE(dy && w && K >= 1 && K <= HEAD_KMAX && C > 0 && (!do_sigmoid || y) && N > 0 && H > 0 &&
              W > 0 && z && coef && mean && invstd && part && pmu_head1x1_bwd_bnr_ok(N, H, W, C));
  PMU_REQUIRE(dw ? (ws != nullptr) : (dl != nullptr && da != nullptr));  // (da null: not stored, dw path only)
  const long long P = (long long)N * H * W;
  const int R = pmu_cdiv(P, HPPB);
  const HeadBnr bn{z, coef, mean, invstd, part, ws};
  if (dw) {  // the head's weight gradient from the same pass (pmu_wgrad1x1's dw, db; dl not written)
    PMU_REQUIRE(ws_bytes >= (size_t)R * K * (C + 1) * sizeof(float));
    const long long HW = (long long)H * W;
    PMU_REQUIRE(head_dispatch(K, do_sigmoid != 0, da != nullptr, [&](auto kt, auto sig, auto stda) {
      hipLaunchKernelGGL((head_bwd_fused_kernel<kt.value, sig.value, stda.value>), dim3((unsigned)R), dim3(256), 0,
                         (hipStream_t)stream, dy, y, w, C, HW, P, da, bn);
    }));
    PMU_CHECK_LAUNCH();
    hipLaunchKernelGGL(rows_sum_split4_kernel, dim3((unsigned)pmu_cdiv(K * (C + 1), 64)), dim3(1024), 0,
                       (hipStream_t)stream, (const float*)ws, R, K, C, dw, db);
  } else {
    hipLaunchKernelGGL((head_bwd_fast_kernel<true, false>), dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, dy, y,
                       do_sigmoid, w, K, C, (long long)H * W, P, dl, da, bn);
  }
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// ---------------- backward applied: the last layer's dz without a stored da ----------------
namespace {
// The last layer's BN+ReLU backward dz from the head's gradient without a stored da (engine.HeadDa):
// da = sum_k g_k w_k formed as head_bwd_fused_kernel forms it (same g, same fmaf order, so the same
// fp32 values), then dz = fmaf(sc, (z*sc+sh > 0) ? da : 0, fmaf(kx, z - mu, kc)) — the frame streams'
// BN-backward formula over bcoef (5 C) — written as bf16 (RNE, the bf16 convs' operand) or fp32 (the
// Winograd input gradient's).  Thread mapping and 4-pixel load batches as head_bwd_fused_kernel.
template <int KT, bool SIG, bool BF>
__global__ __launch_bounds__(256) void head_dz_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                      const float* __restrict__ w, int C, long long HW, long long P,
                                                      const float* __restrict__ z, const float* __restrict__ bcoef,
                                                      void* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int B = 4;
  const int tid = threadIdx.x;
  const int CQ = C >> 2, PG = 256 / CQ;
  const int cq = tid & (CQ - 1), pg = tid / CQ;
  float4 wq[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) wq[k] = *reinterpret_cast<const float4*>(w + k * C + 4 * cq);
  const float4 sc = *reinterpret_cast<const float4*>(bcoef + 4 * cq);
  const float4 sh = *reinterpret_cast<const float4*>(bcoef + C + 4 * cq);
  const float4 mu = *reinterpret_cast<const float4*>(bcoef + 2 * C + 4 * cq);
  const float4 kx = *reinterpret_cast<const float4*>(bcoef + 3 * C + 4 * cq);
  const float4 kc = *reinterpret_cast<const float4*>(bcoef + 4 * C + 4 * cq);
  const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
  const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, kxv[4] = {kx.x, kx.y, kx.z, kx.w}, kcv[4] = {kc.x, kc.y, kc.z, kc.w};
  const unsigned HWu = (unsigned)HW, pend = (unsigned)min(P, (long long)(blockIdx.x + 1) * HPPB);
  // a batch's raw loads (z, dy, and y when SIG), clamped to the block's last pixel; the next batch's are
  // issued before this batch's stores, so waiting for them does not wait (in-order vmcnt) for those stores
  float4 zz[B], zn[B];
  float dyv[B][KT], yv[B][KT], dyn[B][KT], yn[B][KT];
  auto load_batch = [&](unsigned q0, float4 (&zo)[B], float (&dyo)[B][KT], float (&yo)[B][KT])
      __attribute__((always_inline)) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const unsigned p = min(q0 + b * PG, pend - 1);
      const unsigned n = p / HWu, pix = p - n * HWu;
      zo[b] = *reinterpret_cast<const float4*>(z + (size_t)p * C + 4 * cq);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const size_t i = (size_t)(n * KT + k) * HWu + pix;
        dyo[b][k] = dy[i];
        if (SIG) yo[b][k] = y[i];
      }
    }
  };
  const unsigned pfirst = blockIdx.x * HPPB + pg;
  if (pfirst < pend) load_batch(pfirst, zz, dyv, yv);
  for (unsigned p0 = pfirst; p0 < pend; p0 += B * PG) {
    if (p0 + B * PG < pend) load_batch(p0 + B * PG, zn, dyn, yn);
    float g[B][KT];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        g[b][k] = dyv[b][k];
        if (SIG) { const float sg = yv[b][k]; g[b][k] = g[b][k] * (sg * (1.f - sg)); }
      }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const unsigned p = p0 + b * PG;
      if (p >= pend) continue;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        o.x = fmaf(g[b][k], wq[k].x, o.x); o.y = fmaf(g[b][k], wq[k].y, o.y);
        o.z = fmaf(g[b][k], wq[k].z, o.z); o.w = fmaf(g[b][k], wq[k].w, o.w);
      }
      const float ov[4] = {o.x, o.y, o.z, o.w}, zv[4] = {zz[b].x, zz[b].y, zz[b].z, zz[b].w};
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        r[e] = fmaf(scv[e], fmaf(zv[e], scv[e], shv[e]) > 0.f ? ov[e] : 0.f, fmaf(kxv[e], zv[e] - muv[e], kcv[e]));
      if (BF)
        *reinterpret_cast<uint2*>(static_cast<unsigned short*>(out) + (size_t)p * C + 4 * cq) =
            make_uint2(pmu_pk_bf16(r[0], r[1]), pmu_pk_bf16(r[2], r[3]));
      else
        *reinterpret_cast<float4*>(static_cast<float*>(out) + (size_t)p * C + 4 * cq) = make_float4(r[0], r[1], r[2], r[3]);
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      zz[b] = zn[b];
#pragma unroll
      for (int k = 0; k < KT; ++k) { dyv[b][k] = dyn[b][k]; yv[b][k] = yn[b][k]; }
    }
  }
}
}  // namespace

extern "C" int pmu_head1x1_bwd_dz(const float* dy, const float* y, int do_sigmoid, const float* w, int K, int C,
                                  int N, int H, int W, const float* z, const float* bcoef, int out_bf16, void* dz,
                                  void* stream) {
  PMU_REQUIRE(dy && w && K >= 1 && K <= HEAD_KMAX && C > 0 && (!do_sigmoid || y) && N > 0 && H > 0 && W > 0 && z &&
              bcoef && dz && pmu_head1x1_bwd_bnr_ok(N, H, W, C) && (!out_bf16 || C % 8 == 0));
  const long long P = (long long)N * H * W;
  const long long HW = (long long)H * W;
  const int R = pmu_cdiv(P, HPPB);
  PMU_REQUIRE(head_dispatch(K, do_sigmoid != 0, out_bf16 != 0, [&](auto kt, auto sig, auto bf) {
    hipLaunchKernelGGL((head_dz_kernel<kt.value, sig.value, bf.value>), dim3((unsigned)R), dim3(256), 0,
                       (hipStream_t)stream, dy, y, w, C, HW, P, z, bcoef, dz);
  }));
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

// ---------------- weight / bias gradient ----------------
namespace {
// dw[k][c] partial per block: ws[blk][K][C+1] (column C holds the bias grad)
constexpr int W1_PPB = 1024;
__global__ __launch_bounds__(256) void wgrad1x1_kernel(const float* __restrict__ dl, DevFrame f, int K,
                                                       float* __restrict__ ws) {
  __shared__ float red[256 * 33];
  const int tid = threadIdx.x;
  const int C = f.C;
  const int CQ = (C + 3) >> 2;  // quads (CQ <= 64)
  const int npg = 256 / CQ;
  const int q = tid % CQ, pg = tid / CQ;
  const long long HW = (long long)f.H * f.W;
  const long long P = (long long)f.N * HW;
  const long long p0 = (long long)blockIdx.x * W1_PPB;
  float acc[HEAD_KMAX][4];
  float accb[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) { accb[k] = 0.f; for (int e = 0; e < 4; ++e) acc[k][e] = 0.f; }
  if (pg < npg) {
    for (int i = pg; i < W1_PPB; i += npg) {
      const long long p = p0 + i;
      if (p >= P) break;
      const int n = (int)(p / HW);
      const long long pix = p - (long long)n * HW;
      const int ww = (int)(pix % f.W), hh = (int)(pix / f.W);
      const float4 v = frame_value4(f, n, hh, ww, 4 * q);
#pragma unroll
      for (int k = 0; k < HEAD_KMAX; ++k) {
        if (k >= K) break;
        const float g = dl[((long long)n * K + k) * HW + pix];
        acc[k][0] = fmaf(g, v.x, acc[k][0]); acc[k][1] = fmaf(g, v.y, acc[k][1]);
        acc[k][2] = fmaf(g, v.z, acc[k][2]); acc[k][3] = fmaf(g, v.w, acc[k][3]);
        if (q == 0) accb[k] += g;
      }
    }
  }
  const int CW = C + 1;
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) red[tid * 33 + e] = acc[k][e];
    red[tid * 33 + 4] = accb[k];
    __syncthreads();
    if (pg == 0) {
      float t[5] = {0, 0, 0, 0, 0};
      for (int l = 0; l < npg; ++l)
        for (int e = 0; e < 5; ++e) t[e] += red[(l * CQ + q) * 33 + e];
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < C) ws[((long long)blockIdx.x * K + k) * CW + 4 * q + e] = t[e];
      if (q == 0) ws[((long long)blockIdx.x * K + k) * CW + C] = t[4];
    }
    __syncthreads();
  }
}

// dw[k][c] / db[k] partials per block: ws[block][k][C+1]; shuffles over the wave's pixel groups,
// LDS over the 4 waves (fixed order)
__global__ __launch_bounds__(256) void wgrad1x1_fast_kernel(const float* __restrict__ dl, DevFrame f, int K,
                                                            float* __restrict__ ws) {
  __shared__ float red[4 * HEAD_KMAX * 260];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = f.C, CQ = C >> 2, PG = 256 / CQ;
  const int cq = tid & (CQ - 1), pg = tid / CQ;
  const long long HW = (long long)f.H * f.W, P = (long long)f.N * HW;
  const float4 sc = *reinterpret_cast<const float4*>(f.s0.coef + 4 * cq);
  const float4 sh = *reinterpret_cast<const float4*>(f.s0.coef + C + 4 * cq);
  float4 acc[HEAD_KMAX];
  float accb[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); accb[k] = 0.f; }
  const unsigned HWu = (unsigned)HW, pend = (unsigned)min(P, (long long)(blockIdx.x + 1) * HPPB);
  for (unsigned p = blockIdx.x * HPPB + pg; p < pend; p += PG) {  // 32-bit decode (P < 2^31)
    const unsigned n = p / HWu, pix = p - n * HWu;
    const float4 a = pmu_bnrelu4(src_x4(f.s0, (long long)p * C + 4 * cq), sc, sh);
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) {
      if (k >= K) break;
      const float g = dl[(size_t)(n * K + k) * HWu + pix];
      acc[k].x = fmaf(g, a.x, acc[k].x); acc[k].y = fmaf(g, a.y, acc[k].y);
      acc[k].z = fmaf(g, a.z, acc[k].z); acc[k].w = fmaf(g, a.w, acc[k].w);
      accb[k] += g;
    }
  }
  const int CW = C + 1;
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) {
    if (k >= K) break;
    float v[5] = {acc[k].x, acc[k].y, acc[k].z, acc[k].w, accb[k]};
#pragma unroll
    for (int e = 0; e < 5; ++e)
      for (int o = CQ; o < 64; o <<= 1) v[e] += __shfl_xor(v[e], o, 64);
    if (lane < CQ) {  // after the shuffles these lanes hold the wave's sums (all lanes when CQ == 64)
#pragma unroll
      for (int e = 0; e < 4; ++e) red[(wave * HEAD_KMAX + k) * 260 + 4 * cq + e] = v[e];
      if (cq == 0) red[(wave * HEAD_KMAX + k) * 260 + C] = v[4];
    }
  }
  __syncthreads();
  for (int o = tid; o < K * CW; o += 256) {
    const int k = o / CW, c = o - k * CW;
    float t = 0.f;
    for (int wv = 0; wv < 4; ++wv) t += red[(wv * HEAD_KMAX + k) * 260 + c];
    ws[(long long)blockIdx.x * K * CW + o] = t;
  }
}
}  // namespace

extern "C" size_t pmu_wgrad1x1_ws(int P, int K, int C) {
  const int R = pmu_cdiv(P, W1_PPB) > pmu_cdiv(P, HPPB) ? pmu_cdiv(P, W1_PPB) : pmu_cdiv(P, HPPB);
  return (size_t)R * K * (C + 1) * sizeof(float);
}

extern "C" int pmu_wgrad1x1(const float* dl, const pmu_frame* act, int K, float* dw, float* db, float* ws,
                            size_t ws_bytes, void* stream) {
  PMU_REQUIRE(dl && valid_frame(act, true) && dw && ws && K >= 1 && K <= HEAD_KMAX);
  const DevFrame f = make_dev_frame(act);
  PMU_REQUIRE(f.C <= 256);
  const long long P = (long long)act->N * act->H * act->W;
  const bool fast = host_head_fast(act);
  const int R = fast ? pmu_cdiv(P, HPPB) : pmu_cdiv(P, W1_PPB);
  PMU_REQUIRE(ws_bytes >= (size_t)R * K * (f.C + 1) * sizeof(float));
  if (fast)
    hipLaunchKernelGGL(wgrad1x1_fast_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, dl, f, K, ws);
  else
    hipLaunchKernelGGL(wgrad1x1_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, dl, f, K, ws);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(rows_sum_split4_kernel, dim3((unsigned)pmu_cdiv(K * (f.C + 1), 64)), dim3(1024), 0,
                     (hipStream_t)stream, (const float*)ws, R, K, f.C, dw, db);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
