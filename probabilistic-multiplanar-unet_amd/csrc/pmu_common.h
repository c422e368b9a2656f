// Shared device helpers for libpmunet_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/pmunet_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define PMU_CHECK_LAUNCH()                          \
  do {                                              \
    hipError_t e__ = hipGetLastError();             \
    if (e__ != hipSuccess) return (int)e__;         \
  } while (0)
#define PMU_REQUIRE(cond) \
  do {                    \
    if (!(cond)) return PMU_ERR_ARG; \
  } while (0)

static inline int pmu_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// blocks of 256 threads for a grid-stride kernel over n elements (1 .. 8192)
static inline unsigned grid_for(long long n) {
  const long long g = (n + 255) / 256;
  return (unsigned)(g > 8192 ? 8192 : g < 1 ? 1 : g);
}
// class count limit of the 1x1 head and the Dice counters (the ABI's "K <= 8")
constexpr int HEAD_KMAX = 8;
// Column sums of an fp32 slab ws[R][Wd] in fp64, in a fixed order, for the 1024-thread block that owns
// columns [64 b, 64 b + 64): thread (column o, phase ph = tid >> 6 of 16) sums rows ph, ph + 16, ... in
// four interleaved fp64 accumulators (four loads in flight; combined in order), then the 16 phases are
// combined in order through red[1024].  Returns the total in threads tid < 64 (0 elsewhere).  (One
// dependent fp64 add per row with 4 phases left 512-row reductions latency-bound at ~0.2 ms.)
__device__ __forceinline__ double pmu_colsum64x16(const float* __restrict__ ws, int R, int Wd, int o, double* red) {
  const int tid = threadIdx.x, ph = tid >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (o < Wd) {
    int r = ph;
    for (; r + 48 < R; r += 64) {
      a0 += (double)ws[(long long)r * Wd + o];
      a1 += (double)ws[(long long)(r + 16) * Wd + o];
      a2 += (double)ws[(long long)(r + 32) * Wd + o];
      a3 += (double)ws[(long long)(r + 48) * Wd + o];
    }
    for (; r < R; r += 16) a0 += (double)ws[(long long)r * Wd + o];
  }
  red[tid] = ((a0 + a1) + a2) + a3;
  __syncthreads();
  double t = 0.0;
  if (tid < 64)
    for (int p = 0; p < 16; ++p) t += red[p * 64 + tid];
  return t;
}

// compute units of the current device (cached per process: one device per process)
static inline int pmu_num_cus() {
  static const int cus = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return n;
  }();
  return cus;
}

// Kernel-variant switches (PMU_FRAME_NT, PMU_WGW_SDMA: they force a shipped, size-selected path at
// test-sized shapes): read only by `make EXPERIMENTS=1` builds; the shipped library ignores them and
// always dispatches by size.  Launch-shape overrides the tests use to force code paths
// (PMU_*_CPB, *_MINWG, *_BLOCKS) stay plain getenv (pmu_env_int).
static inline const char* pmu_variant_env(const char* name) {
#ifdef PMU_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
// Integer knobs: pmu_env_int for the plain knobs; pmu_variant_int for the variant switches (always dflt in
// the shipped build).
static inline int pmu_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
static inline int pmu_variant_int(const char* name, int dflt) {
  const char* e = pmu_variant_env(name);
  return e ? atoi(e) : dflt;
}

// The LDS-DMA conv kernels address their operand with 32-bit byte offsets.  A launch whose operand
// or output reaches 4 GiB is split over images: f(n0, nn) launches images [n0, n0 + nn), each chunk
// below 4 GiB.  Returns the first error.
template <class F>
static inline int pmu_image_chunks(int N, long long bytes_per_image, F&& f) {
  PMU_REQUIRE(bytes_per_image > 0 && bytes_per_image < (1LL << 32));
  const long long per = ((1LL << 32) - 1) / bytes_per_image;
  for (long long n0 = 0; n0 < N; n0 += per) {
    const int nn = (int)(N - n0 < per ? N - n0 : per);
    const int rc = f((int)n0, nn);
    if (rc) return rc;
  }
  return 0;
}

// Output-channel blocks a Winograd workgroup walks in passes (the per-workgroup prologue is paid once per
// pass group): doubled while at least min_wg workgroups remain; cpb_env > 0 forces a value (A/B, tests).
static inline int pmu_wino_cpb(int nco, long long spatial, int cpb_env, int min_wg) {
  if (cpb_env > 0) return cpb_env < nco ? cpb_env : nco;
  int cpb = 1;
  while (cpb * 2 <= nco && spatial * pmu_cdiv(nco, cpb * 2) >= min_wg) cpb *= 2;
  return cpb;
}

// Host side shared by the Winograd kernels on a materialised NHWC operand (conv3x3_wino2h.hip,
// conv3x3_wino4.hip): one call's operands, and the launch scaffold — argument checks, the split over
// images below 4 GiB, the fields the kernels' args structs have in common (Args: W2Args / W4Args, zeroed
// first) and the cpb choice (env knobs cpb_name / minwg_name, read once per call site).  launch(a,
// spatial, grid) sets what is the kernel's own and launches it.  OW x OH: output pixels per block; CO:
// output channels per block; BK: reduction channels per chunk.
struct pmu_wino_call {
  const float* x;  // [N][H][W][KC]
  int KC, N, H, W;
  const float* wp;
  const float* bias;
  int NOUT;
  float* out0;
  float* out1;
  int split;
  float* part;
  const float* bz;  // input gradient with the producer's BN-backward sums (see W2Args), or null
  const float* bcoef;
  const float* bmean;
  const float* binv;
};
template <class Args, class F>
static inline int pmu_wino_launch(const pmu_wino_call& c, int OW, int OH, int BK, int CO, const char* cpb_name,
                                  const char* minwg_name, F&& launch) {
  PMU_REQUIRE(c.x && c.wp && c.out0 && c.KC > 0 && c.KC % BK == 0 && c.NOUT > 0 && c.N > 0 && c.H > 0 && c.W > 0);
  const long long img_bytes = (long long)c.H * c.W * (c.KC > c.NOUT ? c.KC : c.NOUT) * 4;
  if ((long long)c.N * img_bytes >= (1LL << 32)) {  // 32-bit DMA byte offsets: split over images
    const long long tiles = (long long)pmu_cdiv(c.W, OW) * pmu_cdiv(c.H, OH);
    return pmu_image_chunks(c.N, img_bytes, [&](int n0, int nn) {
      const long long px = (long long)n0 * c.H * c.W;
      pmu_wino_call s = c;
      s.N = nn;
      s.x = c.x + px * c.KC;
      s.out0 = c.out0 + px * c.split;
      s.out1 = c.out1 ? c.out1 + px * (c.NOUT - c.split) : nullptr;
      s.part = c.part ? c.part + (long long)n0 * tiles * 2 * c.NOUT : nullptr;
      s.bz = c.bz ? c.bz + px * c.NOUT : nullptr;
      return pmu_wino_launch<Args>(s, OW, OH, BK, CO, cpb_name, minwg_name, launch);
    });
  }
  Args a;
  memset(&a, 0, sizeof(a));
  a.x = c.x; a.wp = c.wp; a.bias = c.bias; a.out0 = c.out0; a.out1 = c.out1; a.part = c.part;
  a.H = c.H; a.W = c.W; a.KC = c.KC; a.NOUT = c.NOUT; a.split = c.split;
  a.N = c.N;
  a.bz = c.bz; a.bcoef = c.bcoef; a.bmean = c.bmean; a.binv = c.binv;
  a.bw = pmu_cdiv(c.W, OW);
  a.bh = pmu_cdiv(c.H, OH);
  a.nco = pmu_cdiv(c.NOUT, CO);
  const long long spatial = (long long)a.bw * a.bh * c.N;
  static const int cpb_env = pmu_env_int(cpb_name, 0);
  static const int min_wg = pmu_env_int(minwg_name, 1024);
  a.cpb = pmu_wino_cpb(a.nco, spatial, cpb_env, min_wg);
  const long long blocks = (long long)pmu_cdiv(a.nco, a.cpb) * spatial;
  PMU_REQUIRE(blocks < (1LL << 31));
  return launch(a, spatial, dim3((unsigned)blocks));
}

// Batched weight packing (pmu_*_pack_*_multi): one launch packs many tensors of one layout; job j owns
// workgroups [block0, block0 + nblocks) of the grid.
__device__ __forceinline__ int pmu_job_of(const pmu_pack_job* jobs, int njobs, int bid) {
  int j = 0;
  while (j + 1 < njobs && jobs[j + 1].block0 <= bid) ++j;
  return j;
}

// XCD-aware logical block order: the hardware deals consecutive workgroups round-robin over the 8
// XCDs (each with its own L2); the logical id gives every XCD a contiguous range of the nb blocks,
// so a kernel that walks its column blocks fastest re-reads a row block's operand from its own L2.
__device__ __forceinline__ int pmu_xcd_block(int bid, int nb) {
  const int x = bid & 7, q = nb >> 3, r = nb & 7;
  return x * q + (x < r ? x : r) + (bid >> 3);
}
__device__ __forceinline__ int pmu_cdiv_dev(int a, int b) { return (a + b - 1) / b; }

// f32-in / f32-accumulate MFMA: D[32x32] += A[32x2] * B[2x32].
// Lane l supplies A[l&31][l>>5] and B[l>>5][l&31]; D: col = l&31,
// row = (r&3) + 8*(r>>2) + 4*(l>>5) for register r.
__device__ __forceinline__ f32x16 mfma_f32_32x32x2(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ---------------------------------------------------------------------------------
// Operand element loader.  A conv operand is a frame (N x H x W) whose channels are
// the concatenation of up to two sources; each source maps stored values to operand
// values (raw / BN+ReLU / BN+ReLU backward) and may be 2x2-pooled and offset (F.pad).
// Positions outside the frame or the source read as 0 (conv zero padding is applied
// in operand space, i.e. after BN+ReLU, as in the reference).
// ---------------------------------------------------------------------------------
// bf16 storage (pmu_src.dtype): a stored bf16 is read as the fp32 it denotes (exact); conv outputs
// kept in bf16 are rounded to nearest-even
__device__ __forceinline__ float pmu_bf16_f32(unsigned short u) { return __uint_as_float((unsigned)u << 16); }
__device__ __forceinline__ unsigned short pmu_f32_bf16(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }
__device__ __forceinline__ float pmu_round_bf16(float v) { return pmu_bf16_f32(pmu_f32_bf16(v)); }
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));  // a bf16 MFMA operand fragment
typedef short s16x4 __attribute__((ext_vector_type(4)));    // four bf16 as raw bits
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
// ds_read_b64_tr_b16 of channel-contiguous LDS rows (a 16-lane group reads 4 rows x 16 channels and
// receives them column-major), and two such reads as one MFMA operand fragment
__device__ __forceinline__ s16x4 tr_read(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
}
__device__ __forceinline__ bf16x8 frag_of(s16x4 lo, s16x4 hi) {
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// component-wise select (a select of whole uint4 values is lowered through scratch)
__device__ __forceinline__ uint4 keep_if(bool ok, uint4 v) {
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}

// The value of lane l ^ 1 (adjacent-lane swap) as a DPP quad permutation [1, 0, 3, 2]: a VALU move, where
// __shfl_xor(v, 1) is a ds_bpermute whose LDS round trip each use waits for (lgkmcnt(0) per swap in the
// store epilogues).  Every lane of the wave must be active.
__device__ __forceinline__ int pmu_swap1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ unsigned pmu_swap1(unsigned v) { return (unsigned)pmu_swap1((int)v); }
__device__ __forceinline__ float pmu_swap1(float v) {
  return __builtin_bit_cast(float, pmu_swap1(__builtin_bit_cast(int, v)));
}

// Sum over each group of CQ consecutive lanes (CQ a power of two <= 64, wave-uniform; every lane of the
// group gets the total) by DPP moves within 16-lane rows — quad permutations [1,0,3,2], [2,3,0,1], then
// the half-row and row mirrors — and xor shuffles only across rows.  The same operands meet in the same
// order as the xor butterfly (v += v^1, v^2, v^4, v^8, ...): after each step the lanes being combined hold
// equal values, so a mirror partner and an xor partner are interchangeable — bit-identical to it, without
// an LDS round trip (ds_bpermute + lgkmcnt(0)) per step.  Every lane of the wave must be active.
template <int CTRL>
__device__ __forceinline__ float pmu_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float pmu_group_sum(float v, int CQ) {
  if (CQ >= 2) v += pmu_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  if (CQ >= 4) v += pmu_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  if (CQ >= 8) v += pmu_dpp<0x141>(v);  // row_half_mirror
  if (CQ >= 16) v += pmu_dpp<0x140>(v); // row_mirror
  for (int o = 16; o < CQ; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float4 pmu_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 pmu_ld4(const unsigned short* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float pmu_ld1(const float* p) { return *p; }
__device__ __forceinline__ float pmu_ld1(const unsigned short* p) { return pmu_bf16_f32(*p); }

struct DevSrc {
  const float* x;
  const float* z;
  const float* coef;
  int mode, pool, C, H, W, off_h, off_w;
  int xbf, zbf;  // x / z stored as bf16
};
struct DevFrame {
  DevSrc s0, s1;
  int nsrc, N, H, W, C0, C;  // C0 = channels of s0, C = total
  int vec;                   // 1 if every source has C % 4 == 0 (float4 path legal)
};

static inline DevFrame make_dev_frame(const pmu_frame* f) {
  DevFrame d;
  const pmu_src* a = &f->src[0];
  d.s0 = DevSrc{a->x, a->z, a->coef, a->mode, a->pool, a->C, a->H, a->W, a->off_h, a->off_w,
                a->dtype & PMU_DT_X_BF16, (a->dtype & PMU_DT_Z_BF16) >> 1};
  if (f->nsrc > 1) {
    const pmu_src* b = &f->src[1];
    d.s1 = DevSrc{b->x, b->z, b->coef, b->mode, b->pool, b->C, b->H, b->W, b->off_h, b->off_w,
                  b->dtype & PMU_DT_X_BF16, (b->dtype & PMU_DT_Z_BF16) >> 1};
  } else {
    d.s1 = DevSrc{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  }
  d.nsrc = f->nsrc;
  d.N = f->N; d.H = f->H; d.W = f->W;
  d.C0 = a->C;
  d.C = a->C + (f->nsrc > 1 ? f->src[1].C : 0);
  d.vec = (a->C % 4 == 0) && (f->nsrc < 2 || f->src[1].C % 4 == 0);
  return d;
}

static inline bool valid_src(const pmu_src& s, int N) {
  if (!s.x || s.C <= 0 || s.H <= 0 || s.W <= 0) return false;
  if (s.mode == PMU_SRC_BNRELU && !s.coef) return false;
  if (s.mode == PMU_SRC_BNBWD && (!s.coef || !s.z)) return false;
  if (s.mode < 0 || s.mode > 2 || s.pool < 0 || s.pool > 2) return false;
  if (s.dtype < 0 || s.dtype > 3) return false;
  (void)N;
  return true;
}
// bf16: the frame may hold bf16-stored sources (only the calls whose kernels read sources through
// src_xform / src_xform4 pass true; the fused-staging kernels read fp32 and refuse them)
static inline bool valid_frame(const pmu_frame* f, bool bf16 = false) {
  if (!f || f->nsrc < 1 || f->nsrc > 2 || f->N <= 0 || f->H <= 0 || f->W <= 0) return false;
  for (int i = 0; i < f->nsrc; ++i) {
    if (!valid_src(f->src[i], f->N)) return false;
    if (!bf16 && f->src[i].dtype != 0) return false;
    const pmu_src& s = f->src[i];
    if (s.pool == PMU_POOL_MAX2 && (s.H / 2 + s.off_h > f->H || s.W / 2 + s.off_w > f->W)) return false;
  }
  return true;
}

// transform of one stored element (index i into x/z, channel c of the source)
__device__ __forceinline__ float src_x1(const DevSrc& s, long long i) {
  return s.xbf ? pmu_ld1(reinterpret_cast<const unsigned short*>(s.x) + i) : s.x[i];
}
__device__ __forceinline__ float4 src_x4(const DevSrc& s, long long i) {
  return s.xbf ? pmu_ld4(reinterpret_cast<const unsigned short*>(s.x) + i) : pmu_ld4(s.x + i);
}
__device__ __forceinline__ float src_xform(const DevSrc& s, long long i, int c) {
  const float x = src_x1(s, i);
  if (s.mode == PMU_SRC_RAW) return x;
  if (s.mode == PMU_SRC_BNRELU) return fmaxf(0.f, fmaf(x, s.coef[c], s.coef[s.C + c]));
  // BNBWD
  const float z = s.zbf ? pmu_ld1(reinterpret_cast<const unsigned short*>(s.z) + i) : s.z[i];
  const float sc = s.coef[c];
  const float g = (fmaf(z, sc, s.coef[s.C + c]) > 0.f) ? x : 0.f;
  return fmaf(sc, g, fmaf(s.coef[3 * s.C + c], z - s.coef[2 * s.C + c], s.coef[4 * s.C + c]));
}
__device__ __forceinline__ float4 src_xform4(const DevSrc& s, long long i, int c) {
  const float4 x = src_x4(s, i);
  if (s.mode == PMU_SRC_RAW) return x;
  const float4 sc = *reinterpret_cast<const float4*>(s.coef + c);
  const float4 sh = *reinterpret_cast<const float4*>(s.coef + s.C + c);
  if (s.mode == PMU_SRC_BNRELU) {
    return make_float4(fmaxf(0.f, fmaf(x.x, sc.x, sh.x)), fmaxf(0.f, fmaf(x.y, sc.y, sh.y)),
                       fmaxf(0.f, fmaf(x.z, sc.z, sh.z)), fmaxf(0.f, fmaf(x.w, sc.w, sh.w)));
  }
  const float4 z = s.zbf ? pmu_ld4(reinterpret_cast<const unsigned short*>(s.z) + i) : pmu_ld4(s.z + i);
  const float4 mu = *reinterpret_cast<const float4*>(s.coef + 2 * s.C + c);
  const float4 kx = *reinterpret_cast<const float4*>(s.coef + 3 * s.C + c);
  const float4 kc = *reinterpret_cast<const float4*>(s.coef + 4 * s.C + c);
  float4 r;
  r.x = fmaf(sc.x, fmaf(z.x, sc.x, sh.x) > 0.f ? x.x : 0.f, fmaf(kx.x, z.x - mu.x, kc.x));
  r.y = fmaf(sc.y, fmaf(z.y, sc.y, sh.y) > 0.f ? x.y : 0.f, fmaf(kx.y, z.y - mu.y, kc.y));
  r.z = fmaf(sc.z, fmaf(z.z, sc.z, sh.z) > 0.f ? x.z : 0.f, fmaf(kx.z, z.z - mu.z, kc.z));
  r.w = fmaf(sc.w, fmaf(z.w, sc.w, sh.w) > 0.f ? x.w : 0.f, fmaf(kx.w, z.w - mu.w, kc.w));
  return r;
}

// value of source s at source-frame position (hs, ws) (already offset-corrected), channel c
__device__ __forceinline__ float src_value(const DevSrc& s, int n, int hs, int ws, int c) {
  if (s.pool == PMU_POOL_NONE) {
    if (hs < 0 || ws < 0 || hs >= s.H || ws >= s.W) return 0.f;
    return src_xform(s, (((long long)n * s.H + hs) * s.W + ws) * s.C + c, c);
  }
  const int h0 = 2 * hs, w0 = 2 * ws;
  // floor mode (max): a window starting on the odd last row / column of the source is no window — the frame
  // may be larger than the pooled source; ceil mode (avg): a partial window counts
  const int whole = s.pool == PMU_POOL_MAX2 ? 1 : 0;
  if (hs < 0 || ws < 0 || h0 + whole >= s.H || w0 + whole >= s.W) return 0.f;
  if (s.pool == PMU_POOL_MAX2) {  // the whole window is inside
    const long long b = (((long long)n * s.H + h0) * s.W + w0) * s.C + c;
    const long long rs = (long long)s.W * s.C;
    float m = src_xform(s, b, c);
    m = fmaxf(m, src_xform(s, b + s.C, c));
    m = fmaxf(m, src_xform(s, b + rs, c));
    m = fmaxf(m, src_xform(s, b + rs + s.C, c));
    return m;
  }
  // avg 2x2, ceil mode, divisor = number of in-bounds elements
  const int h1 = min(h0 + 2, s.H), w1 = min(w0 + 2, s.W);
  float acc = 0.f;
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) acc += src_xform(s, (((long long)n * s.H + h) * s.W + w) * s.C + c, c);
  return acc / (float)((h1 - h0) * (w1 - w0));
}
__device__ __forceinline__ float4 src_value4(const DevSrc& s, int n, int hs, int ws, int c) {
  if (s.pool == PMU_POOL_NONE) {
    if (hs < 0 || ws < 0 || hs >= s.H || ws >= s.W) return make_float4(0.f, 0.f, 0.f, 0.f);
    return src_xform4(s, (((long long)n * s.H + hs) * s.W + ws) * s.C + c, c);
  }
  const int h0 = 2 * hs, w0 = 2 * ws;
  const int whole = s.pool == PMU_POOL_MAX2 ? 1 : 0;  // (as src_value)
  if (hs < 0 || ws < 0 || h0 + whole >= s.H || w0 + whole >= s.W) return make_float4(0.f, 0.f, 0.f, 0.f);
  if (s.pool == PMU_POOL_MAX2) {
    const long long b = (((long long)n * s.H + h0) * s.W + w0) * s.C + c;
    const long long rs = (long long)s.W * s.C;
    float4 a = src_xform4(s, b, c), t;
    t = src_xform4(s, b + s.C, c);
    a.x = fmaxf(a.x, t.x); a.y = fmaxf(a.y, t.y); a.z = fmaxf(a.z, t.z); a.w = fmaxf(a.w, t.w);
    t = src_xform4(s, b + rs, c);
    a.x = fmaxf(a.x, t.x); a.y = fmaxf(a.y, t.y); a.z = fmaxf(a.z, t.z); a.w = fmaxf(a.w, t.w);
    t = src_xform4(s, b + rs + s.C, c);
    a.x = fmaxf(a.x, t.x); a.y = fmaxf(a.y, t.y); a.z = fmaxf(a.z, t.z); a.w = fmaxf(a.w, t.w);
    return a;
  }
  const int h1 = min(h0 + 2, s.H), w1 = min(w0 + 2, s.W);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) {
      const float4 t = src_xform4(s, (((long long)n * s.H + h) * s.W + w) * s.C + c, c);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
  const float inv = 1.f / (float)((h1 - h0) * (w1 - w0));
  acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
  return acc;
}

// frame element (n, h, w, c); c may be >= C (returns 0)
__device__ __forceinline__ float frame_value(const DevFrame& f, int n, int h, int w, int c) {
  if (c >= f.C || h < 0 || w < 0 || h >= f.H || w >= f.W) return 0.f;
  if (c < f.C0) return src_value(f.s0, n, h - f.s0.off_h, w - f.s0.off_w, c);
  return src_value(f.s1, n, h - f.s1.off_h, w - f.s1.off_w, c - f.C0);
}
// 4 consecutive channels c..c+3 (c % 4 == 0); uses the vector path when legal
__device__ __forceinline__ float4 frame_value4(const DevFrame& f, int n, int h, int w, int c) {
  if (h < 0 || w < 0 || h >= f.H || w >= f.W || c >= f.C) return make_float4(0.f, 0.f, 0.f, 0.f);
  if (f.vec && c + 3 < f.C) {
    if (c < f.C0) return src_value4(f.s0, n, h - f.s0.off_h, w - f.s0.off_w, c);
    return src_value4(f.s1, n, h - f.s1.off_h, w - f.s1.off_w, c - f.C0);
  }
  return make_float4(frame_value(f, n, h, w, c), frame_value(f, n, h, w, c + 1),
                     frame_value(f, n, h, w, c + 2), frame_value(f, n, h, w, c + 3));
}

// Split-K slab reduction shared by the weight-gradient kernels: dw[cc*9 + tap] = sum over sp of
// ws[sp][tap][cc] (E = 9*CC elements per slab).  A 256-thread block owns 64 consecutive elements;
// its 4 waves each sum the splits sp = g, g+4, ... (4 independent accumulators, combined in a fixed
// order) and wave 0 adds the 4 partials in order: deterministic, 4x the loads in flight of one
// thread per element walking all splits.
static __global__ __launch_bounds__(256) void pmu_splitk_reduce9_kernel(const float* __restrict__ ws, int nsplit,
                                                                       long long CC, float* __restrict__ dw) {
  __shared__ float red[4][64];
  const long long E = 9 * CC;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long e = (long long)blockIdx.x * 64 + lane;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < E) {
    int sp = g;
    for (; sp + 12 < nsplit; sp += 16) {
      s0 += ws[(long long)sp * E + e];
      s1 += ws[(long long)(sp + 4) * E + e];
      s2 += ws[(long long)(sp + 8) * E + e];
      s3 += ws[(long long)(sp + 12) * E + e];
    }
    for (; sp < nsplit; sp += 4) s0 += ws[(long long)sp * E + e];
  }
  red[g][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && e < E) {
    const float t = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    const int tap = (int)(e / CC);
    dw[(e - tap * CC) * 9 + tap] = t;
  }
}

// wave-level sum over 64 lanes
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- bounds-checked debug build ------------------------------------------------------------
// `make DEBUG=1` builds libpmunet_hip_debug.so with -DPMU_DEBUG: PMU_DCHECK(cond, code) records the
// first violated index bound of each translation unit (code, source line, workgroup) in a device
// global and lets the kernel continue — it never traps (a trapping kernel faults the device).  The
// host reads the records with pmu_debug_read() (include/pmunet_hip.h; tests/conftest.py checks them
// after every GPU test when the debug library is loaded).  The shipped library compiles the checks
// out entirely.
#define PMU_DBG_OPERAND 1   // operand read / DMA source outside the operand tensor
#define PMU_DBG_OUTPUT 2    // store outside the output tensor
#define PMU_DBG_GRID 3      // a workgroup mapped outside the problem (batch, tile or channel block)
#define PMU_DBG_INDEX 4     // a data-dependent index (label, slice id, class) outside its range
#define PMU_DBG_WORKSPACE 5 // split-K slab / partial-sum row outside the workspace
#ifdef PMU_DEBUG
static __device__ int pmu_dbg_rec[4];   // {code, line, workgroup, set}
__device__ __attribute__((noinline)) static void pmu_dbg_fail(int code, int line) {
  if (atomicCAS(&pmu_dbg_rec[3], 0, 1) == 0) {
    pmu_dbg_rec[0] = code;
    pmu_dbg_rec[1] = line;
    pmu_dbg_rec[2] = (int)blockIdx.x;
  }
}
#define PMU_DCHECK(cond, code)                 \
  do {                                         \
    if (!(cond)) pmu_dbg_fail((code), __LINE__); \
  } while (0)
int pmu_dbg_register(const char* tu, int (*rd)(int*), int (*rs)());
static int pmu_dbg_read_tu(int* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pmu_dbg_rec), sizeof(pmu_dbg_rec));
}
static int pmu_dbg_reset_tu() {
  const int z[4] = {0, 0, 0, 0};
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(pmu_dbg_rec), z, sizeof(z));
}
static const int pmu_dbg_registered __attribute__((unused)) =
    pmu_dbg_register(__FILE__, pmu_dbg_read_tu, pmu_dbg_reset_tu);
#else
#define PMU_DCHECK(cond, code) \
  do {                         \
  } while (0)
#endif
