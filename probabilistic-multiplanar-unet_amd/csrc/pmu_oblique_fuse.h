// A voxel seen from one oblique view, shared by the plain-mean fusion (oblique.hip pmu_fuse_oblique) and the
// learned fusion (fusion_fit.hip pmu_fusion_oblique_eval): the map of the voxel into the view's grid, the
// coverage rule and the fp32 trilinear read of the view's probability stack.  Geometry: DESIGN.md, "Oblique
// views".  FP contraction is off (the pragma below, whatever the including file's include order), so
// both kernels compute a view's resampled probability as the same bits, and tests/oblique_ref.py restates it.
#pragma once
#include "pmu_common.h"
#include "pmu_sample.h"

#pragma clang fp contract(off)

namespace {

// p[0], p[1] in one load (p is 4-byte aligned only); second: both results are p[1]
__device__ __forceinline__ float2 ld_pair(const float* p, bool second) {
  float2 r;
  __builtin_memcpy(&r, p, sizeof(r));
  if (second) r.x = r.y;
  return r;
}

// The interpolation cell of a covered voxel in a P^3 stack: [s0, s1] x [a0, a1] x [bb, bb + 1] with the fp32
// weights of the upper neighbours.
struct ObliqueCell {
  int s0, s1;
  long long o0, o1;   // a0 * P + bb, a1 * P + bb
  float ws, wa, wb;
  bool last;          // b0 == P - 1: both W-neighbours are the second element of the pair at bb
};

// Voxel offset (d0, d1, d2) from the volume's centre in the grid of the view with frame f[9]: true iff the
// view covers it (0 <= g <= P-1 on all three axes), and then its cell.
__device__ __forceinline__ bool oblique_cell(const double* f, double d0, double d1, double d2, double h, int P,
                                             bool valid, ObliqueCell& q) {
  const double half = (double)(P - 1) / 2.0;
  const double gs = ((d0 * f[0] + d1 * f[1]) + d2 * f[2]) / h + half;
  const double ga = ((d0 * f[3] + d1 * f[4]) + d2 * f[5]) / h + half;
  const double gb = ((d0 * f[6] + d1 * f[7]) + d2 * f[8]) / h + half;
  const double top = (double)(P - 1);
  const bool cov = valid && gs >= 0.0 && gs <= top && ga >= 0.0 && ga <= top && gb >= 0.0 && gb <= top;
  if (cov) {
    // (under the condition, not for every lane: the branch-free form keeps fuse_oblique_kernel at 78 VGPRs and 6
    // waves per SIMD where this one takes 92 and 5, and measured 8 % slower: DESIGN.md, "Learned fusion")
    // cell [s0, s1] x [a0, a1] x [b0, b1]; on the last grid plane the upper neighbour is the
    // plane itself and the weight 0, so a grid point is read back exactly
    const double fs = floor(gs), fa = floor(ga), fb = floor(gb);
    const int s0 = (int)fs, a0 = (int)fa, b0 = (int)fb;
    const int a1 = min(a0 + 1, P - 1);
    q.s0 = s0;
    q.s1 = min(s0 + 1, P - 1);
    q.ws = (float)(gs - fs);
    q.wa = (float)(ga - fa);
    q.wb = (float)(gb - fb);
    // the two W-neighbours are adjacent in memory: one 8-byte load at bb = min(b0, P-2) fetches both
    // (on the last column, where the upper neighbour is b0 itself, both are its second element)
    const int bb = min(b0, P - 2);
    q.last = b0 != bb;
    PMU_DCHECK(s0 >= 0 && q.s1 < P && a0 >= 0 && a1 < P && bb >= 0 && bb + 1 < P, PMU_DBG_OPERAND);
    q.o0 = (long long)a0 * P + bb;
    q.o1 = (long long)a1 * P + bb;
  }
  return cov;
}

// Class c of the view's stack st [P][C][P][P] at the cell: a + w (b - a) along W, H, then the slice axis.
__device__ __forceinline__ float oblique_prob(const float* __restrict__ st, const ObliqueCell& q, int C, int c,
                                              long long P2) {
  const float* q0 = st + ((long long)q.s0 * C + c) * P2;
  const float* q1 = st + ((long long)q.s1 * C + c) * P2;
  const float2 r00 = ld_pair(q0 + q.o0, q.last), r01 = ld_pair(q0 + q.o1, q.last);
  const float2 r10 = ld_pair(q1 + q.o0, q.last), r11 = ld_pair(q1 + q.o1, q.last);
  const float x00 = r00.x + q.wb * (r00.y - r00.x);
  const float x01 = r01.x + q.wb * (r01.y - r01.x);
  const float x10 = r10.x + q.wb * (r10.y - r10.x);
  const float x11 = r11.x + q.wb * (r11.y - r11.x);
  const float y0 = x00 + q.wa * (x01 - x00);
  const float y1 = x10 + q.wa * (x11 - x10);
  return y0 + q.ws * (y1 - y0);
}

__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__ballot(pred)); }

}  // namespace
