// Per-voxel pieces of the view fusion shared by the plain-mean kernels (data.hip pmu_fuse3view, oblique.hip
// pmu_fuse_oblique) and the learned fusion (fusion_fit.hip): the class and view limits of the ABI, the fp32
// softmax over the classes and the first-maximum label.  One definition, so a view's probabilities and its
// label are the same bits in every kernel that fuses it.
#pragma once
#include "pmu_common.h"

namespace {

constexpr int FUSE_CMAX = 8;
constexpr int FUSE_VMAX = 8;

// register arrays of CB (<= FUSE_CMAX) entries, only the first C live: every loop is unrolled and guarded
template <int CB>
__device__ __forceinline__ int argmax_first(const float (&p)[CB], int C) {
  int am = 0;
  float best = p[0];
#pragma unroll
  for (int c = 1; c < CB; ++c)
    if (c < C && p[c] > best) { best = p[c]; am = c; }
  return am;
}

template <int CB>
__device__ __forceinline__ void softmax_inplace(float (&p)[CB], int C) {
  float m = p[0];
#pragma unroll
  for (int c = 1; c < CB; ++c)
    if (c < C) m = fmaxf(m, p[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) { p[c] = expf(p[c] - m); s += p[c]; }
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) p[c] = p[c] / s;
}

}  // namespace
