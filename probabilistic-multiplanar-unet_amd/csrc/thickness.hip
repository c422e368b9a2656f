// Local thickness (Hildebrand & Ruegsegger): the covering pass pmu_local_thickness over the interior distance
// field of pmu_interior_edt (surface.hip).  pmu_hip/thickness.py builds the thickness map and the per-class
// volume / thickness numbers on them.
//
// d2 fp32 [D0][D1][D2]: D2(q) > 0 on the structure (the squared distance of q to the nearest voxel outside it),
// 0 elsewhere.  The open ball of q holds every voxel p with d2(p, q) < D2(q), where, as in surface.hip,
//     t_i = fl(fl(s_i * float(e_i)) * fl(s_i * float(e_i))),    d2(p, q) = fl(fl(t_2 + t_1) + t_0),
// every operation a single rounding (__fmul_rn / __fadd_rn, FP contraction off for the file).  The result is
//     R2(p) = max{ D2(q) : D2(q) > 0, d2(p, q) < D2(q) }   for D2(p) > 0,   0 elsewhere:
// the squared radius of the largest ball that fits inside the structure and contains p.  It is a maximum of input
// values, so it does not depend on the order of evaluation: the same bits on every run, and the numpy
// restatement tests/thickness_ref.py computes the same bits.
//
//   thick_tilemax_kernel  one block per TH x TH x TH tile: the tile's maximum of D2 into the coarse grid tmax, and
//                         the volume's maximum by an integer atomicMax on the float bits (D2 >= 0: the bit
//                         patterns order like the values).
//   thick_cover_kernel    one 512-thread block per tile of output voxels, one voxel per thread; best = D2(p), the
//                         voxel's own ball.  The block walks the source tiles inside the reach of the volume's
//                         maximum and skips a source tile outright when
//                           - its maximum is 0 (nothing of the structure in it),
//                           - its maximum is not above the smallest best of the output tile (no ball of it can
//                             raise any voxel), or
//                           - the box-to-box gap g of the two tiles has fl(fl(t_2(g_2) + t_1(g_1)) + t_0(g_0)) >=
//                             its maximum: every pair (p, q) of the tiles has |e_i| >= g_i, t_i is non-decreasing
//                             and fp32 addition of a non-negative term is monotone, so d2(p, q) >= the gap value
//                             >= D2(q) and no ball of the tile reaches the output tile.
//                         The box is walked in four sweeps of falling tile maximum (a partition of the positive
//                         values by fractions of the volume's maximum), so the deep tiles, whose balls cover
//                         most, raise the bests before the shallow ones are looked at.
//                         A tile that survives is staged in LDS with axis 0 contiguous, so that the eight source
//                         voxels q of one (q1, q2) are two 16-byte broadcast reads.  A wave (one axis-0 plane of
//                         the output tile) leaves the tile out when its maximum is not above the wave's smallest
//                         best or the gap test fails with the plane's own gap along axis 0.  A group of eight is
//                         the same for every lane, and it is skipped (a wave-uniform branch) unless one of its D2
//                         is above the wave's smallest best and above the gap value of its row q1 to the wave.
//                         Per pair that is left: one addition, one comparison, one maximum and one select; t_2
//                         and t_0 of the eight offsets sit in registers, fl(t_2 + t_1) is shared by the eight q
//                         of a group.
// Every skip drops only pairs that cannot change the maximum (D2(q) not above the current best of any voxel
// concerned, or a lower bound of d2(p, q) that is not below D2(q)); the result is exact.
#include "pmu_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH = PMU_THICKNESS_TILE;     // tile edge
constexpr int TH_V = TH * TH * TH;         // 512 voxels, one thread each
constexpr int TH_MAXDIM = PMU_SURFACE_MAX_DIM;
static_assert(TH == 8 && TH_V == 512, "a wave holds one axis-0 plane of the tile; two float4 per (q1, q2) group");

__device__ __forceinline__ float sq_step(float s, int d) {
  const float a = __fmul_rn(s, (float)d);
  return __fmul_rn(a, a);
}
__device__ __forceinline__ float dist2(float t2, float t1, float t0) { return __fadd_rn(__fadd_rn(t2, t1), t0); }
__device__ __forceinline__ int iabs(int a) { return a < 0 ? -a : a; }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

struct Tiles {
  int n0, n1, n2;
};

// D2 of voxel (i0, i1, i2), 0 outside the volume and wherever the field is not positive (a NaN included)
__device__ __forceinline__ float load_d2(const float* __restrict__ d2, int D0, int D1, int D2, int i0, int i1,
                                         int i2) {
  if (i0 >= D0 || i1 >= D1 || i2 >= D2) return 0.f;
  PMU_DCHECK(i0 >= 0 && i1 >= 0 && i2 >= 0, PMU_DBG_OPERAND);
  const float v = d2[((long long)i0 * D1 + i1) * D2 + i2];
  return v > 0.f ? v : 0.f;
}

__global__ __launch_bounds__(TH_V) void thick_tilemax_kernel(const float* __restrict__ d2, int D0, int D1, int D2,
                                                             Tiles nt, float* __restrict__ tmax,
                                                             unsigned* __restrict__ gmax) {
  __shared__ float wm[TH_V / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int b0 = b / (nt.n1 * nt.n2), b1 = (b / nt.n2) % nt.n1, b2 = b % nt.n2;
  PMU_DCHECK(b0 < nt.n0, PMU_DBG_GRID);
  const float v = load_d2(d2, D0, D1, D2, b0 * TH + (tid >> 6), b1 * TH + ((tid >> 3) & 7), b2 * TH + (tid & 7));
  const float w = wave_max(v);
  if ((tid & 63) == 0) wm[tid >> 6] = w;
  __syncthreads();
  if (tid == 0) {
    float m = wm[0];
#pragma unroll
    for (int i = 1; i < TH_V / 64; ++i) m = fmaxf(m, wm[i]);
    tmax[b] = m;
    if (m > 0.f) atomicMax(gmax, __float_as_uint(m));
  }
}

// Tiles an index distance of at most this many voxels can span, from the edge of a tile
__device__ __forceinline__ int reach_tiles(float m, float s, int D) {
  // t(e) <= d2(p, q) < D2(q) <= m needs s * e < sqrt(m) up to rounding in the seventh digit; e <= 1023
  float e = __fdiv_rn(__fsqrt_rn(m), s) + 2.f;
  if (!(e < (float)D)) e = (float)D;  // (also an infinite or NaN estimate)
  return ((int)e + TH - 1) / TH;
}

__global__ __launch_bounds__(TH_V) void thick_cover_kernel(const float* __restrict__ d2, int D0, int D1, int D2,
                                                           float s0, float s1, float s2, Tiles nt,
                                                           const float* __restrict__ tmax,
                                                           const unsigned* __restrict__ gmax,
                                                           float* __restrict__ r2) {
  __shared__ __attribute__((aligned(16))) float src[TH_V];  // [q1][q2][q0]
  __shared__ float wmin[TH_V / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int b0 = b / (nt.n1 * nt.n2), b1 = (b / nt.n2) % nt.n1, b2 = b % nt.n2;
  PMU_DCHECK(b0 < nt.n0, PMU_DBG_GRID);
  const int l0 = tid >> 6, l1 = (tid >> 3) & 7, l2 = tid & 7;  // a wave: one l0, the 8 x 8 (l1, l2)
  const int p0 = b0 * TH + l0, p1 = b1 * TH + l1, p2 = b2 * TH + l2;
  const bool in_vol = p0 < D0 && p1 < D1 && p2 < D2;
  const long long pv = ((long long)p0 * D1 + p1) * D2 + p2;
  const float inf = __builtin_inff();
  if (tmax[b] == 0.f) {  // block-uniform: nothing of the structure in this tile
    if (in_vol) {
      PMU_DCHECK(pv < (long long)D0 * D1 * D2, PMU_DBG_OUTPUT);
      r2[pv] = 0.f;
    }
    return;
  }
  const float own = load_d2(d2, D0, D1, D2, p0, p1, p2);
  float best = own > 0.f ? own : inf;  // a voxel off the structure needs nothing: it never lowers a minimum
  const float gm = __uint_as_float(*gmax);
  const int rt0 = reach_tiles(gm, s0, D0), rt1 = reach_tiles(gm, s1, D1), rt2 = reach_tiles(gm, s2, D2);
  const int a0 = b0 - rt0 < 0 ? 0 : b0 - rt0, e0 = b0 + rt0 >= nt.n0 ? nt.n0 - 1 : b0 + rt0;
  const int a1 = b1 - rt1 < 0 ? 0 : b1 - rt1, e1 = b1 + rt1 >= nt.n1 ? nt.n1 - 1 : b1 + rt1;
  const int a2 = b2 - rt2 < 0 ? 0 : b2 - rt2, e2 = b2 + rt2 >= nt.n2 ? nt.n2 - 1 : b2 + rt2;
  float block_thr = 0.f;  // the smallest best of the output tile, as of the last staged tile
  // Four sweeps over the box, by falling tile maximum: [gm/2, inf), [gm/4, gm/2), [gm/16, gm/4), (0, gm/16) — a
  // partition of the positive values, so every tile is taken in exactly one sweep.  The deep tiles come first and
  // raise the bests, and most of the shallow ones then fail the second skip.
  for (int sweep = 0; sweep < 4; ++sweep) {
    const float hi = sweep == 0 ? inf : __fmul_rn(gm, sweep == 1 ? 0.5f : sweep == 2 ? 0.25f : 0.0625f);
    const float lo = sweep == 3 ? 0.f : __fmul_rn(gm, sweep == 0 ? 0.5f : sweep == 1 ? 0.25f : 0.0625f);
    if (!(hi > block_thr)) break;  // (block-uniform) nothing below hi can raise a voxel
    for (int c0 = a0; c0 <= e0; ++c0) {
      const int k0 = iabs(c0 - b0);
      const float g0 = sq_step(s0, k0 ? (k0 - 1) * TH + 1 : 0);
      // the gap along axis 0 between the wave's plane p0 and the source tile (wave-uniform)
      const int w0 = c0 * TH > p0 ? c0 * TH - p0 : p0 > c0 * TH + TH - 1 ? p0 - (c0 * TH + TH - 1) : 0;
      const float g0w = sq_step(s0, w0);
      for (int c1 = a1; c1 <= e1; ++c1) {
        const int k1 = iabs(c1 - b1);
        const float g1 = sq_step(s1, k1 ? (k1 - 1) * TH + 1 : 0);
        for (int c2 = a2; c2 <= e2; ++c2) {
          const int k2 = iabs(c2 - b2);
          const float g2 = sq_step(s2, k2 ? (k2 - 1) * TH + 1 : 0);
          const int c = (c0 * nt.n1 + c1) * nt.n2 + c2;
          const float tm = tmax[c];
          // block-uniform: every thread reads the same words
          if (tm == 0.f || !(tm >= lo && tm < hi) || !(tm > block_thr) || dist2(g2, g1, g0) >= tm) continue;
          __syncthreads();  // the reads of the tile staged before are done
          src[(l1 * TH + l2) * TH + l0] = load_d2(d2, D0, D1, D2, c0 * TH + l0, c1 * TH + l1, c2 * TH + l2);
          const float wthr = wave_min(best);
          if ((tid & 63) == 0) wmin[tid >> 6] = wthr;
          __syncthreads();
          block_thr = wmin[0];
#pragma unroll
          for (int i = 1; i < TH_V / 64; ++i) block_thr = fminf(block_thr, wmin[i]);
          // wave-uniform (no barrier below): no ball of the tile can raise a voxel of this wave, or reach its plane
          if (!(tm > wthr) || dist2(g2, g1, g0w) >= tm) continue;
          float t0r[TH], t2r[TH];
#pragma unroll
          for (int a = 0; a < TH; ++a) {
            t0r[a] = sq_step(s0, iabs(c0 * TH + a - p0));
            t2r[a] = sq_step(s2, iabs(c2 * TH + a - p2));
          }
          for (int q1 = 0; q1 < TH; ++q1) {
            const int j1 = c1 * TH + q1;
            const float t1 = sq_step(s1, iabs(j1 - p1));
            // the least d2 of a voxel of this wave to row q1 of the tile: the row's gap to the output tile along
            // axis 1, the tiles' gap along axis 2, the plane's along axis 0 (wave-uniform)
            const int w1 = j1 < b1 * TH ? b1 * TH - j1 : j1 > b1 * TH + TH - 1 ? j1 - (b1 * TH + TH - 1) : 0;
            const float row_gap = dist2(g2, sq_step(s1, w1), g0w);
#pragma unroll
            for (int q2 = 0; q2 < TH; ++q2) {
              const float4 A = *reinterpret_cast<const float4*>(src + (q1 * TH + q2) * TH);
              const float4 B = *reinterpret_cast<const float4*>(src + (q1 * TH + q2) * TH + 4);
              const float D[TH] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
              const float mx = fmaxf(fmaxf(fmaxf(D[0], D[1]), fmaxf(D[2], D[3])),
                                     fmaxf(fmaxf(D[4], D[5]), fmaxf(D[6], D[7])));
              // wave-uniform: the group is the same for every lane
              if (!(mx > wthr) || row_gap >= mx) continue;
              const float u = __fadd_rn(t2r[q2], t1);
#pragma unroll
              for (int a = 0; a < TH; ++a) {
                const float d = __fadd_rn(u, t0r[a]);
                best = d < D[a] ? fmaxf(best, D[a]) : best;
              }
            }
          }
        }
      }
    }
  }
  if (in_vol) {
    PMU_DCHECK(pv < (long long)D0 * D1 * D2, PMU_DBG_OUTPUT);
    r2[pv] = own > 0.f ? best : 0.f;
  }
}

bool dims_ok(int D0, int D1, int D2) {
  if (D0 < 1 || D0 > TH_MAXDIM || D1 < 1 || D1 > TH_MAXDIM || D2 < 1 || D2 > TH_MAXDIM) return false;
  return (long long)D0 * D1 * D2 < (1LL << 31);
}
bool spacing_ok(float s) { return s > 0.f && s <= 3.402823466e38f; }  // finite and positive (NaN fails both)
Tiles tiles_of(int D0, int D1, int D2) { return {(D0 + TH - 1) / TH, (D1 + TH - 1) / TH, (D2 + TH - 1) / TH}; }

}  // namespace

extern "C" size_t pmu_local_thickness_ws(int D0, int D1, int D2) {
  if (!dims_ok(D0, D1, D2)) return 0;
  const Tiles nt = tiles_of(D0, D1, D2);
  return ((size_t)nt.n0 * nt.n1 * nt.n2 + 1) * sizeof(float);  // the volume's maximum, then the tile maxima
}

extern "C" int pmu_local_thickness(const float* d2, int D0, int D1, int D2, float s0, float s1, float s2, float* r2,
                                   void* ws, size_t ws_bytes, void* stream) {
  PMU_REQUIRE(d2 && r2 && ws && dims_ok(D0, D1, D2));
  PMU_REQUIRE(spacing_ok(s0) && spacing_ok(s1) && spacing_ok(s2));
  PMU_REQUIRE(ws_bytes >= pmu_local_thickness_ws(D0, D1, D2));
  hipStream_t st = (hipStream_t)stream;
  const Tiles nt = tiles_of(D0, D1, D2);
  const unsigned blocks = (unsigned)(nt.n0 * nt.n1 * nt.n2);  // <= 2^31 / 512 + the partial tiles
  unsigned* gmax = (unsigned*)ws;
  float* tmax = (float*)ws + 1;
  if (hipMemsetAsync(gmax, 0, sizeof(unsigned), st) != hipSuccess) return PMU_ERR_ARG;
  hipLaunchKernelGGL(thick_tilemax_kernel, dim3(blocks), dim3(TH_V), 0, st, d2, D0, D1, D2, nt, tmax, gmax);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(thick_cover_kernel, dim3(blocks), dim3(TH_V), 0, st, d2, D0, D1, D2, s0, s1, s2, nt, tmax, gmax,
                     r2);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
