// 3x3 / pad 1 convolution in fp32 by Winograd F(2x2, 3x3), high-occupancy variant: the forward of
// nn.Conv2d at PMU/model/unet/unet_parts.py:15,18 (and its input gradient) on a materialised NHWC
// operand, the same arithmetic as conv3x3_wino.hip's kernels (16 products per 2x2 tile per channel
// pair; transforms with coefficients 0, +-1, +-1/2; results equal the direct sum to fp32 rounding).
//
// Block: 1024 threads = 16 waves, four per SIMD (the weight gradient measured 12% faster going from
// two to four waves per SIMD): 64 tiles (8 x 8 -> a 16 x 16 output patch) x 64 output channels.
// Wave w = (tile group tg = w & 3: tile rows 2tg, 2tg+1; component half ch = (w >> 2) & 1: rows
// 2ch, 2ch+1 of the 4x4 component grid; channel group cg = w >> 3: 32 outputs).  A wave keeps 8
// components x 2 co halves = 16 f32x4 accumulators (64 registers, < 128 in all), forms only its half
// of V = B^T d B (16 VALU for 16 MFMAs) and the two component halves of a tile group swap partial
// outputs through a free LDS stage in the epilogue.  Per chunk of 8 input channels (two MFMA steps),
// double-buffered stages receive the 18 x 18 x 8 operand image (2-pixel groups + a pad unit) and U
// (8 ch x 64 co x 16 comps, units swizzled by u_swz) by LDS-DMA; the patch is read per chunk as 12
// ds_read_b64 channel pairs (w2_pair).
#include <string.h>
#include <stdlib.h>
#include "pmu_common.h"
#include "pmu_lds.h"

namespace {

constexpr int TX = 8, TY = 8;                 // tiles per block
constexpr int OW = 2 * TX, OH = 2 * TY;       // 16 x 16 output pixels
constexpr int HW = OW + 2, HH = OH + 2;       // 18 x 18 halo
constexpr int BK = 8;                         // input channels per chunk
constexpr int GP = 20;                        // floats per group of 2 halo pixels (2 x 8 ch + 1 pad unit)
constexpr int ROWF = 208;                     // floats per halo row (9 groups = 180, padded to 16 mod 32:
                                              // the wave's two tile rows 2 ROWF = 32 mod 64 floats apart,
                                              // conflict-free ds_read_b64 patch pairs, see w2_pair)
constexpr int ROWU = ROWF / 4;
constexpr int A_FLOATS = HH * ROWF;
[[maybe_unused]] constexpr int NC = 16;       // Winograd components
constexpr int NCP = 16;                       // floats per U row: the 16 components as four 16-B units, unit q
                                              // of row r stored at q ^ u_swz(r) (the lanes' b128 U reads
                                              // conflict-free without a pad unit, see u_swz)
constexpr int A_UNITS = A_FLOATS / 4;

// U row r = kl * CO + co (channel in chunk, output channel in block) keeps its 16-B unit q at q ^ u_swz(r):
// 16 lanes reading rows r .. r + 15 (one b128 phase) then cover the 64 banks once — rows 4 apart, 256 B
// = 64 banks apart, land on different units.  Every lane's row is 32 cg + 16 h + t (+ CO per channel, CO a
// multiple of 16), so u_swz(row) = (t >> 2) & 3 for the lane's t = lane & 15.
__host__ __device__ constexpr int u_swz(int row) { return (row >> 2) & 3; }

// block geometry: 64 output channels per block (1024 threads, 16 waves, one block per CU)
constexpr int CO = 64;
constexpr int NT = 16 * CO;
constexpr int NW = NT / 64;
constexpr int U_FLOATS = BK * CO * NCP;          // [ch 8][co][comp 16, units swizzled]
constexpr int STAGE = A_FLOATS + U_FLOATS;
constexpr int NGL = (A_UNITS + NT - 1) / NT;
constexpr int UGL = (U_FLOATS / 4 + NT - 1) / NT;  // U DMA rounds (the last one by the first waves)
constexpr int RED_FLOATS = NW * 16 * 2;
constexpr int XB_FLOATS = NW * 2 * 4 * 64;         // one exchange round: waves x 2 tiles x 4 outputs x lanes
static_assert(U_FLOATS % (4 * 64) == 0, "U of whole wave DMA instructions");
static_assert(XB_FLOATS <= STAGE, "exchange round fits a stage");
static_assert((2 * STAGE + RED_FLOATS) * 4 <= 160 * 1024, "LDS");

struct W2Args {
  const float* x;     // [N][H][W][KC]
  const float* wp;    // packed U [co block][chunk][ch 8][co 64][comp 16, units swizzled by u_swz]
  const float* bias;
  float* out0;
  float* out1;
  float* part;        // [spatial blocks][2][NOUT] BN partial sums (fwd) or null
  int H, W, KC, NOUT, split, bw, bh, nco, cpb;
  int N;              // images (bounds checks of the debug build)
  // input gradient only: BatchNorm+ReLU backward partial sums of the layer that produced the operand
  // of this conv (dx is that layer's da): part[spatial][2][NOUT] += (sum g, sum g*xhat) with
  // g = dx * (z*scale+shift > 0), xhat = (z-mean)*invstd (pmu_bn_bwd_reduce's sums); null: none
  const float* bz;
  const float* bcoef;
  const float* bmean;
  const float* binv;
};

__device__ __forceinline__ void wino2_u(const float (&g)[3][3], float (&u)[16]) {
  float t[4][3];
  for (int b = 0; b < 3; ++b) {
    t[0][b] = g[0][b];
    t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
    t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
    t[3][b] = g[2][b];
  }
  for (int a = 0; a < 4; ++a) {
    u[4 * a + 0] = t[a][0];
    u[4 * a + 1] = 0.5f * (t[a][0] + t[a][1] + t[a][2]);
    u[4 * a + 2] = 0.5f * (t[a][0] - t[a][1] + t[a][2]);
    u[4 * a + 3] = t[a][2];
  }
}

// U = G g G^T, G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]; one thread per (co block, chunk,
// channel, co) writes its 16 components (c = 4a + b) as 4 float4 (input-gradient packing: consecutive
// threads read consecutive filters w[co][ci..])
__device__ __forceinline__ void pack_wino2h_body(const float* __restrict__ w, int Cout, int Cin, int dgrad,
                                                 float* __restrict__ wp, int bid, int nblk) {
  const int NOUT = dgrad ? Cin : Cout, KC = dgrad ? Cout : Cin;
  const int nch = (KC + BK - 1) / BK, ncob = (NOUT + CO - 1) / CO;
  const long long total = (long long)ncob * nch * BK * CO;
  for (long long e = (long long)bid * blockDim.x + threadIdx.x; e < total; e += (long long)nblk * blockDim.x) {
    const int col = (int)(e % CO);
    long long r = e / CO;
    const int kl = (int)(r % BK); r /= BK;
    const int ch = (int)(r % nch);
    const int jb = (int)(r / nch);
    const int j = jb * CO + col, k = ch * BK + kl;
    float g[3][3];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        float v = 0.f;
        if (j < NOUT && k < KC)  // dgrad: the input gradient convolves dz with w[co][ci] rotated by 180 degrees
          v = dgrad ? w[((long long)k * Cin + j) * 9 + (2 - a) * 3 + (2 - b)] : w[((long long)j * Cin + k) * 9 + a * 3 + b];
        g[a][b] = v;
      }
    float u[16];
    wino2_u(g, u);
    float* dst = wp + (((long long)jb * nch + ch) * BK + kl) * (CO * NCP) + col * NCP;
    const int sw = u_swz(kl * CO + col);
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(dst + 4 * (q ^ sw)) = make_float4(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]);
  }
}
__global__ void pack_wino2h_kernel(const float* __restrict__ w, int Cout, int Cin, int dgrad, float* __restrict__ wp) {
  pack_wino2h_body(w, Cout, Cin, dgrad, wp, blockIdx.x, gridDim.x);
}

// Forward packing, one workgroup per (co block, chunk): the 8 x CO filters w[co][ci0..ci0+7] are read
// along ci (8 lanes cover 288 contiguous bytes), transformed into LDS in the packed order, and the
// workgroup's contiguous BK x CO x NCP segment is stored with consecutive float4s.
__device__ __forceinline__ void pack_wino2h_fwd_body(const float* __restrict__ w, int Cout, int Cin,
                                                     float* __restrict__ wp, int bid) {
  constexpr int SEG = BK * CO * NCP;
  __shared__ float4 seg4[SEG / 4];
  const int nch = (Cin + BK - 1) / BK;
  const int ch = bid % nch, jb = bid / nch;
  for (int f = threadIdx.x; f < BK * CO; f += blockDim.x) {
    const int kl = f % BK, col = f / BK;
    const int j = jb * CO + col, k = ch * BK + kl;
    float g[3][3];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) g[a][b] = (j < Cout && k < Cin) ? w[((long long)j * Cin + k) * 9 + a * 3 + b] : 0.f;
    float u[16];
    wino2_u(g, u);
    float4* d = seg4 + (kl * CO + col) * (NCP / 4);
    const int sw = u_swz(kl * CO + col);
    for (int q = 0; q < 4; ++q) d[q ^ sw] = make_float4(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]);
  }
  __syncthreads();
  float4* dst = reinterpret_cast<float4*>(wp + (long long)bid * SEG);
  for (int i = threadIdx.x; i < SEG / 4; i += blockDim.x) dst[i] = seg4[i];
}
__global__ __launch_bounds__(256) void pack_wino2h_fwd_kernel(const float* __restrict__ w, int Cout, int Cin,
                                                              float* __restrict__ wp) {
  pack_wino2h_fwd_body(w, Cout, Cin, wp, blockIdx.x);
}
__global__ __launch_bounds__(256) void pack_wino2h_multi_kernel(const pmu_pack_job* __restrict__ jobs, int njobs,
                                                                int dgrad) {
  const pmu_pack_job& j = jobs[pmu_job_of(jobs, njobs, blockIdx.x)];
  const int bid = blockIdx.x - j.block0;
  if (dgrad) pack_wino2h_body(j.w, j.Cout, j.Cin, 1, (float*)j.dst, bid, j.nblocks);
  else pack_wino2h_fwd_body(j.w, j.Cout, j.Cin, (float*)j.dst, bid);
}

// patch element (i, j) of this lane's tile: byte offset from the patch origin
#define PMU_W2P(I, J) ((((I) * ROWF) + ((J) >> 1) * GP + ((J) & 1) * 8) * 4)

// half CH of B^T d B from the column-pass halves t[a][j] (a = 0, 1): v[4a + b]
__device__ __forceinline__ void w2_rows(const float (&t)[2][4], float (&v)[8]) {
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    v[4 * a + 0] = t[a][0] - t[a][2];
    v[4 * a + 1] = t[a][1] + t[a][2];
    v[4 * a + 2] = t[a][2] - t[a][1];
    v[4 * a + 3] = t[a][1] - t[a][3];
  }
}

// 16 MFMAs of one step on v with U groups (u00, u10) and (u01, u11); the second group waited for here
// (W: lgkmcnt allowing the reads issued after it)
template <int W>
__device__ __forceinline__ void w2_mfma(const float (&v)[8], float4 u00, float4 u10, float4 u01, float4 u11,
                                        f32x4 (&acc)[2][8]) {
  acc[0][0] = mfma16(v[0], u00.x, acc[0][0]);
  acc[1][0] = mfma16(v[0], u10.x, acc[1][0]);
  acc[0][1] = mfma16(v[1], u00.y, acc[0][1]);
  acc[1][1] = mfma16(v[1], u10.y, acc[1][1]);
  acc[0][2] = mfma16(v[2], u00.z, acc[0][2]);
  acc[1][2] = mfma16(v[2], u10.z, acc[1][2]);
  acc[0][3] = mfma16(v[3], u00.w, acc[0][3]);
  acc[1][3] = mfma16(v[3], u10.w, acc[1][3]);
  __builtin_amdgcn_sched_barrier(0);
  wait_lgkm<W>();
  __builtin_amdgcn_sched_barrier(0);
  acc[0][4] = mfma16(v[4], u01.x, acc[0][4]);
  acc[1][4] = mfma16(v[4], u11.x, acc[1][4]);
  acc[0][5] = mfma16(v[5], u01.y, acc[0][5]);
  acc[1][5] = mfma16(v[5], u11.y, acc[1][5]);
  acc[0][6] = mfma16(v[6], u01.z, acc[0][6]);
  acc[1][6] = mfma16(v[6], u11.z, acc[1][6]);
  acc[0][7] = mfma16(v[7], u01.w, acc[0][7]);
  acc[1][7] = mfma16(v[7], u11.w, acc[1][7]);
  __builtin_amdgcn_sched_barrier(0);
}

// Both MFMA steps of a chunk (channels 2kk, 2kk + 1 of k-slot kk) with the patch read as ds_read_b64
// channel pairs, and only the three patch rows this component half uses (rows CH .. CH + 2): 12 b64 reads
// per chunk.  Bank map of a 32-lane group (b64: dword banks mod 64): tile columns
// GP = 20 floats apart, the wave's two tile rows 2 ROWF = 32 (mod 64) apart, the k-slot pair 2 floats:
// the 16 tiles x 2 k-slots cover the 64 banks once.
template <int CH>
__device__ __forceinline__ void w2_pair(unsigned pa, unsigned ua0, f32x4 (&acc)[2][8]) {
  float2 c[3][4];
#define PMU_RD2(I, J) c[I][J] = lds_b64<PMU_W2P(CH + (I), J)>(pa);
  PMU_RD2(0, 0) PMU_RD2(0, 1) PMU_RD2(0, 2) PMU_RD2(0, 3) PMU_RD2(1, 0) PMU_RD2(1, 1) PMU_RD2(1, 2) PMU_RD2(1, 3)
  PMU_RD2(2, 0) PMU_RD2(2, 1) PMU_RD2(2, 2) PMU_RD2(2, 3)
#undef PMU_RD2
  wait_lgkm<0>();  // the patch
  __builtin_amdgcn_sched_barrier(0);
  // column pass (rows CH .. CH+2 of d as c[0..2]): CH 0: (d0 - d2, d1 + d2); CH 1: (d2 - d1, d1 - d3)
  float t0[2][4], t1[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (CH == 0) {
      t0[0][j] = c[0][j].x - c[2][j].x;
      t0[1][j] = c[1][j].x + c[2][j].x;
      t1[0][j] = c[0][j].y - c[2][j].y;
      t1[1][j] = c[1][j].y + c[2][j].y;
    } else {
      t0[0][j] = c[1][j].x - c[0][j].x;
      t0[1][j] = c[0][j].x - c[2][j].x;
      t1[0][j] = c[1][j].y - c[0][j].y;
      t1[1][j] = c[0][j].y - c[2][j].y;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // U after the patch is consumed (at the 128-register cap of four waves per SIMD the patch pairs and U
  // together spilled; the SIMD's other waves cover the U read latency)
  // (unit 2CH + 1 at ua0 ^ 16, formed at each use: one register fewer live across the MFMAs)
  float4 u00 = lds_b128<0>(ua0);
  float4 u10 = lds_b128<16 * NCP * 4>(ua0);
  float4 u01 = lds_b128<0>(ua0 ^ 16u);
  float4 u11 = lds_b128<16 * NCP * 4>(ua0 ^ 16u);
  float v[8];
  w2_rows(t0, v);
  wait_lgkm<2>();  // U group 0
  __builtin_amdgcn_sched_barrier(0);
  w2_mfma<0>(v, u00, u10, u01, u11, acc);
  const unsigned ub = ua0 + CO * NCP * 4;  // step 1: the next channel's rows, CO rows on (same swizzle)
  u00 = lds_b128<0>(ub);
  u10 = lds_b128<16 * NCP * 4>(ub);
  u01 = lds_b128<0>(ub ^ 16u);
  u11 = lds_b128<16 * NCP * 4>(ub ^ 16u);
  w2_rows(t1, v);
  wait_lgkm<2>();  // step 1's U group 0
  __builtin_amdgcn_sched_barrier(0);
  w2_mfma<0>(v, u00, u10, u01, u11, acc);
}

// this half's share of Y = A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]) for tile r of co half h:
// P[2p + q] = sum over the half's rows a of A^T[p][a] (M[a][:] A)[q]
template <int CH>
__device__ __forceinline__ void w2_partial(const f32x4 (&acc)[2][8], int h, int r, float (&P)[4]) {
  float R[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const float m0 = acc[h][4 * a][r], m1 = acc[h][4 * a + 1][r], m2 = acc[h][4 * a + 2][r], m3 = acc[h][4 * a + 3][r];
    R[a][0] = m0 + m1 + m2;
    R[a][1] = m1 - m2 - m3;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (CH == 0) {  // rows 0, 1: A^T columns (1, 0), (1, 1)
      P[q] = R[0][q] + R[1][q];
      P[2 + q] = R[1][q];
    } else {        // rows 2, 3: A^T columns (1, -1), (0, -1)
      P[q] = R[0][q];
      P[2 + q] = -R[0][q] - R[1][q];
    }
  }
}

// epilogue: lane holds M[comp (half CH)][tile 4*kk + r of the group][co j0 + 32 cg + 16 h + (lane & 15)];
// the two component halves of (tg, cg) swap the partial outputs of the co half the other finishes
// through xb (a free LDS stage), in two rounds of two tiles per lane
template <bool DGRAD, bool BNR, int CH>
__device__ __forceinline__ void wino2h_epilogue(const W2Args& a, int n, int h0, int w0, int j0, int spatial,
                                                const f32x4 (&acc)[2][8], float* xb, float* red, float bias) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4;
  const int tg = wave & 3, cg = wave >> 3, partner = tg + 4 * (1 - CH) + 8 * cg;
  const int j = j0 + 32 * cg + 16 * CH + (lane & 15);
  const bool jok = j < a.NOUT;
  // this lane's output column: the forward's z, or the input gradient's dx0 / dx1 side of the split
  float* dst;
  int ld;
  if (!DGRAD) { dst = a.out0 + j; ld = a.NOUT; }
  else if (j < a.split) { dst = a.out0 + j; ld = a.split; }
  else { dst = a.out1 + (j - a.split); ld = a.NOUT - a.split; }
  float s1 = 0.f, s2 = 0.f;
  float bsc = 0.f, bsh = 0.f, bmu = 0.f, bis = 0.f;
  if (BNR && jok) {
    bsc = a.bcoef[j];
    bsh = a.bcoef[a.NOUT + j];
    bmu = a.bmean[j];
    bis = a.binv[j];
  }
  // (BNR) the producer's z under a round's two tiles (4 outputs each), loaded at the start of the round,
  // before its stores: loaded per tile between the stores, each tile's z waited (in-order vmcnt) for
  // every earlier store of the epilogue — four HBM round trips per wave behind the stores, now one (the
  // second round's).  All four tiles' z up front spilled 18 VGPRs.  Clamped addresses: every lane loads,
  // unused values are ignored.
  float zt2[2][4];
#pragma unroll
  for (int rho = 0; rho < 2; ++rho) {
    if (BNR) {
      const int jc = min(j, a.NOUT - 1);
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int t = 4 * kk + 2 * rho + rr;
        const int oh = h0 + 2 * (2 * tg + (t >> 3)), ow = w0 + 2 * (t & 7);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long pix = ((long long)n * a.H + min(oh + (e >> 1), a.H - 1)) * a.W + min(ow + (e & 1), a.W - 1);
          zt2[rr][e] = a.bz[pix * a.NOUT + jc];
        }
      }
    }
    if (rho) __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      float P[4];
      w2_partial<CH>(acc, 1 - CH, 2 * rho + rr, P);
#pragma unroll
      for (int e = 0; e < 4; ++e) xb[((wave * 2 + rr) * 4 + e) * 64 + lane] = P[e];
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * rho + rr;
      const int t = 4 * kk + r;
      const int oh = h0 + 2 * (2 * tg + (t >> 3)), ow = w0 + 2 * (t & 7);
      const float (&zt)[4] = zt2[rr];
      float P[4];
      w2_partial<CH>(acc, CH, r, P);
      // the partner's partial outputs read together and held in registers before any store branch (read
      // where used, the plain input gradient's ds_reads sank into the store branches, each followed by
      // an lgkmcnt(0): serial LDS round trips).  Values, masks and BN sums are formed unconditionally
      // and only the stores are predicated: a global-memory value (bias, z) first consumed inside a
      // per-output branch made the compiler wait vmcnt(0) in every branch, i.e. for every earlier store
      // of the epilogue to complete.
      float xv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[e] = xb[((partner * 2 + rr) * 4 + e) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(xv[e]));
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int hh = oh + p;
        float* rowp = dst + (long long)((long long)n * a.H + min(hh, a.H - 1)) * a.W * ld;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int ww = ow + q;
          const float v = P[2 * p + q] + xv[2 * p + q] + bias;
          const bool ok = jok && hh < a.H && ww < a.W;
          if (!DGRAD) {
            const float m = ok ? v : 0.f;
            s1 += m;
            s2 = fmaf(m, m, s2);
          } else if (BNR) {
            const float zz = zt[2 * p + q];
            const float g = (ok && fmaf(zz, bsc, bsh) > 0.f) ? v : 0.f;
            s1 += g;
            s2 = fmaf(g, (zz - bmu) * bis, s2);
          }
          if (!ok) continue;
          PMU_DCHECK((((long long)n * a.H + hh) * a.W + ww) < (long long)a.N * a.H * a.W && j < a.NOUT, PMU_DBG_OUTPUT);
          rowp[(unsigned)(ww * ld)] = v;
        }
      }
    }
  }
  if (a.part) {  // forward: BN partial sums of the output; input gradient: of the producer's BN backward
    s1 += __shfl_xor(s1, 16, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (lane < 16) {
      red[(wave * 16 + lane) * 2 + 0] = s1;
      red[(wave * 16 + lane) * 2 + 1] = s2;
    }
    __syncthreads();
    if (tid < CO) {  // channel tid = 32 cg + 16 h + l, summed over the 4 tile groups in order
      const int jj = j0 + tid, cgg = tid >> 5, hf = (tid >> 4) & 1, l = tid & 15;
      if (jj < a.NOUT) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int wv = g + 4 * hf + 8 * cgg;
          t1 += red[(wv * 16 + l) * 2 + 0];
          t2 += red[(wv * 16 + l) * 2 + 1];
        }
        PMU_DCHECK(spatial < (long long)a.N * a.bh * a.bw, PMU_DBG_WORKSPACE);
        a.part[((long long)spatial * 2 + 0) * a.NOUT + jj] = t1;
        a.part[((long long)spatial * 2 + 1) * a.NOUT + jj] = t2;
      }
    }
  }
  __syncthreads();  // the exchange reads are done before the next pass reuses xb's stage
}

struct W2Block {
  int n, h0, w0, cob0, spatial, nchunks, npass;
  unsigned gin, gzero;
};

template <bool DGRAD, bool BNR, int CH>
__device__ __forceinline__ void wino2h_main(const W2Args& a, const W2Block& B, const unsigned (&goff)[NGL],
                                            float* smem) {
  float* red = smem + 2 * STAGE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nchunks = B.nchunks, total = B.npass * nchunks;
  const float* wsrc = a.wp + (long long)B.cob0 * nchunks * U_FLOATS;
  const unsigned uoff = 16u * tid;
  const int wave_off = wave * 256;
  const unsigned gin = B.gin;
  // serpentine chunk order over the passes (as conv3x3_wino4.hip): a pass begins on the chunks the
  // previous one fetched last, still in L2; direction by co-block parity (independent of cpb)
#define PMU_FETCH2(GI, BUF)                                                                                 \
  {                                                                                                        \
    const int p_ = (GI) / nchunks;                                                                         \
    const int c_ = (GI) - p_ * nchunks;                                                                    \
    const int cs_ = ((B.cob0 + p_) & 1) ? nchunks - 1 - c_ : c_;                                           \
    const int k0_ = cs_ * BK;                                                                              \
    PMU_DCHECK(k0_ + BK <= a.KC, PMU_DBG_OPERAND);                                                         \
    float* b_ = (BUF);                                                                                     \
    const char* xb_ = reinterpret_cast<const char*>(a.x + k0_);                                            \
    _Pragma("unroll") for (int r = 0; r < NGL; ++r)                                                        \
      if ((gin >> r) & 1u) PMU_GLDS(xb_ + goff[r], b_ + 4 * (r * NT) + wave_off)                           \
    const char* s_ = reinterpret_cast<const char*>(wsrc + ((long long)p_ * nchunks + cs_) * U_FLOATS) + uoff; \
    float* d_ = b_ + A_FLOATS + wave_off;                                                                  \
    _Pragma("unroll") for (int r = 0; r < UGL; ++r)                                                        \
      if (r * NT * 4 + (wave + 1) * 256 <= U_FLOATS) PMU_GLDS(s_ + 16 * NT * r, d_ + 4 * NT * r)          \
  }
  const int t = lane & 15, kk = lane >> 4, tg = wave & 3, cg = wave >> 3;
  const int pbase = 2 * (2 * tg + (t >> 3)) * ROWF + GP * (t & 7) + 2 * kk;
  const int ubase = A_FLOATS + (2 * kk * CO + 32 * cg + t) * NCP;
  static_assert(CO % 16 == 0, "u_swz of every row a lane reads is (t >> 2) & 3");
  // byte offset of unit 2CH of the lane's row in a stage; unit 2CH + 1 is at that ^ 16 (rows 64-B aligned:
  // smem aligned to 64, A_FLOATS and STAGE multiples of 16 floats)
  const unsigned uoff0 = 4u * ubase + 16u * ((2 * CH) ^ ((t >> 2) & 3));
  f32x4 acc[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[h][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  PMU_FETCH2(0, smem)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int p = 0; p < B.npass; ++p) {
    const int j0 = (B.cob0 + p) * CO;
    const int jb = j0 + 32 * cg + 16 * CH + t;
    const float bias = (!DGRAD && a.bias && jb < a.NOUT) ? a.bias[jb] : 0.f;
    int gi = p * nchunks;
    for (int ch = 0; ch < nchunks; ++ch, ++gi) {
      float* cur = smem + (gi & 1) * STAGE;
      if (gi + 1 < total) PMU_FETCH2(gi + 1, smem + ((gi + 1) & 1) * STAGE)
      const unsigned pa = lds_addr(cur + pbase), ua0 = lds_addr(cur) + uoff0;
      w2_pair<CH>(pa, ua0, acc);                         // channels 2*kk, 2*kk + 1
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next chunk's DMA has landed
      __syncthreads();
    }
    int ne = B.n, h0e = B.h0, w0e = B.w0;
    asm volatile("" : "+s"(ne), "+s"(h0e), "+s"(w0e));
    float* xb = smem + ((gi - 1) & 1) * STAGE;
    wino2h_epilogue<DGRAD, BNR, CH>(a, ne, h0e, w0e, j0, B.spatial, acc, xb, red, bias);
    if (p + 1 < B.npass) {  // block-uniform: restore the zero units the exchange overwrote
#pragma unroll
      for (int r = 0; r < NGL; ++r)
        if ((B.gzero >> r) & 1u) *reinterpret_cast<float4*>(xb + 4 * (r * NT + tid)) = make_float4(0.f, 0.f, 0.f, 0.f);
      __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[h][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#undef PMU_FETCH2
}

// BNR (input gradient only): the producer's BN-backward partial sums in the epilogue (a.bz set) — a
// compile-time choice, so the z loads and their uses sit in straight-line code
// 1024 threads = four waves per SIMD (<= 128 VGPRs implied)
template <bool DGRAD, bool BNR>
__global__ __launch_bounds__(NT, 1) void conv3x3_wino2h_kernel(W2Args a) {
  __shared__ __attribute__((aligned(64))) float smem[2 * STAGE + RED_FLOATS];
  static_assert(A_FLOATS % 16 == 0 && STAGE % 16 == 0, "U rows 64-B aligned (ua1 = ua0 ^ 16)");
  const int tid = threadIdx.x;
  const int lb = pmu_xcd_block(blockIdx.x, gridDim.x);
  const int ncog = (a.nco + a.cpb - 1) / a.cpb;
  W2Block B;
  B.cob0 = (lb % ncog) * a.cpb;
  int sp = lb / ncog;
  B.spatial = sp;
  const int bx = sp % a.bw; sp /= a.bw;
  const int by = sp % a.bh;
  B.n = sp / a.bh;
  B.h0 = by * OH;
  B.w0 = bx * OW;
  const int KC = a.KC;
  B.nchunks = KC / BK;
  B.npass = a.cpb < a.nco - B.cob0 ? a.cpb : a.nco - B.cob0;
  PMU_DCHECK(B.n < a.N && B.cob0 < a.nco, PMU_DBG_GRID);
  unsigned goff[NGL];
  unsigned gin = 0u, gzero = 0u;
#pragma unroll
  for (int r = 0; r < NGL; ++r) {
    const int u = r * NT + tid;
    const int hr = u / ROWU, wu = u - hr * ROWU;
    const int g = wu / 5, w5 = wu - 5 * g;
    const int px = 2 * g + (w5 >> 1);
    const bool data = u < A_UNITS && w5 < 4 && px < HW;
    const int h = B.h0 - 1 + hr, w = B.w0 - 1 + px;
    const bool in = data && h >= 0 && w >= 0 && h < a.H && w < a.W;
    goff[r] = in ? (unsigned)(((((long long)B.n * a.H + h) * a.W + w) * KC + 4 * (w5 & 1)) * 4) : 0u;
    PMU_DCHECK(!in || (((long long)B.n * a.H + h) * a.W + w) < (long long)a.N * a.H * a.W, PMU_DBG_OPERAND);
    gin |= in ? (1u << r) : 0u;
    gzero |= (data && !in) ? (1u << r) : 0u;
    if (data && !in) {
      *reinterpret_cast<float4*>(smem + 4 * u) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(smem + STAGE + 4 * u) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  B.gin = gin;
  B.gzero = gzero;
  if ((tid >> 8) & 1) wino2h_main<DGRAD, BNR, 1>(a, B, goff, smem);
  else wino2h_main<DGRAD, BNR, 0>(a, B, goff, smem);
}

int launch_wino2h(const float* x, int KC, int N, int H, int W, const float* wp, const float* bias, int NOUT,
                  float* out0, float* out1, int split, float* part, bool dgrad, void* stream,
                 const float* bz = nullptr, const float* bcoef = nullptr, const float* bmean = nullptr,
                 const float* binv = nullptr) {
  const pmu_wino_call c{x, KC, N, H, W, wp, bias, NOUT, out0, out1, split, part, bz, bcoef, bmean, binv};
  return pmu_wino_launch<W2Args>(c, OW, OH, BK, CO, "PMU_WINO2H_CPB", "PMU_WINO2H_MINWG",
                                 [&](const W2Args& a, long long, dim3 grid) {
    hipStream_t st = (hipStream_t)stream;
    const bool bnr = dgrad && bz;
    if (bnr) hipLaunchKernelGGL((conv3x3_wino2h_kernel<true, true>), grid, dim3(NT), 0, st, a);
    else if (dgrad) hipLaunchKernelGGL((conv3x3_wino2h_kernel<true, false>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((conv3x3_wino2h_kernel<false, false>), grid, dim3(NT), 0, st, a);
    PMU_CHECK_LAUNCH();
    return (int)PMU_OK;
  });
}

}  // namespace

extern "C" int pmu_conv3x3_tiles_wino2h(int N, int H, int W) { return N * pmu_cdiv(H, OH) * pmu_cdiv(W, OW); }

extern "C" size_t pmu_conv3x3_packed_size_wino2h(int Cout, int Cin, int dgrad) {
  const int NOUT = dgrad ? Cin : Cout, KC = dgrad ? Cout : Cin;
  return (size_t)pmu_cdiv(NOUT, CO) * pmu_cdiv(KC, BK) * U_FLOATS * sizeof(float);
}

extern "C" int pmu_conv3x3_pack_wino2h(const float* w, int Cout, int Cin, int dgrad, float* wp, void* stream) {
  PMU_REQUIRE(w && wp && Cout > 0 && Cin > 0);
  const long long total = (long long)pmu_conv3x3_packed_size_wino2h(Cout, Cin, dgrad) / sizeof(float) / NCP;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipStream_t st = (hipStream_t)stream;
  // forward: one workgroup per (co block, chunk) segment
  const unsigned segs = (unsigned)(pmu_cdiv(Cout, CO) * pmu_cdiv(Cin, BK));
  if (!dgrad) hipLaunchKernelGGL(pack_wino2h_fwd_kernel, dim3(segs), dim3(256), 0, st, w, Cout, Cin, wp);
  else hipLaunchKernelGGL(pack_wino2h_kernel, dim3(blocks), dim3(256), 0, st, w, Cout, Cin, dgrad, wp);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_conv3x3_fwd_wino2h(const float* xt, int Cin, int N, int H, int W, const float* wp, const float* bias,
                                      int Cout, float* z, float* part, void* stream) {
  return launch_wino2h(xt, Cin, N, H, W, wp, bias, Cout, z, nullptr, Cout, part, false, stream);
}

extern "C" int pmu_conv3x3_dgrad_wino2h(const float* dzt, int Cout, int N, int H, int W, const float* wp, int Cin,
                                        int Csplit, float* dx0, float* dx1, void* stream) {
  PMU_REQUIRE(Csplit > 0 && Csplit <= Cin && (Csplit == Cin || dx1));
  return launch_wino2h(dzt, Cout, N, H, W, wp, nullptr, Cin, dx0, dx1, Csplit, nullptr, true, stream);
}

// As pmu_conv3x3_dgrad_wino4_bnr (part rows = pmu_conv3x3_tiles_wino2h).
extern "C" int pmu_conv3x3_dgrad_wino2h_bnr(const float* dzt, int Cout, int N, int H, int W, const float* wp, int Cin,
                                            float* dx, const float* z, const float* coef, const float* mean,
                                            const float* invstd, float* part, void* stream) {
  PMU_REQUIRE(z && coef && mean && invstd && part);
  return launch_wino2h(dzt, Cout, N, H, W, wp, nullptr, Cin, dx, nullptr, Cin, part, true, stream, z, coef, mean,
                       invstd);
}

static int pack_wino2h_grid(int Cout, int Cin, int dgrad) {
  if (!dgrad) return pmu_cdiv(Cout, CO) * pmu_cdiv(Cin, BK);
  const long long total = (long long)pmu_conv3x3_packed_size_wino2h(Cout, Cin, dgrad) / sizeof(float) / NCP;
  return (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
}

extern "C" int pmu_conv3x3_pack_wino2h_blocks(int Cout, int Cin, int dgrad) { return pack_wino2h_grid(Cout, Cin, dgrad); }

extern "C" int pmu_conv3x3_pack_wino2h_multi(const pmu_pack_job* jobs, int njobs, int blocks, int dgrad, void* stream) {
  PMU_REQUIRE(jobs && njobs > 0 && blocks > 0);
  hipLaunchKernelGGL(pack_wino2h_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, jobs, njobs,
                     dgrad);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
