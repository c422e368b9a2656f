// The on-the-fly sampler of a resident padded fp64 volume, shared by the oblique-view kernels (oblique.hip)
// and the warped batch gather (augment.hip).  Geometry: DESIGN.md, "Oblique views".  Every coordinate is
// evaluated in one order with FP contraction off (the pragma below stays in force for the rest of the
// including file), so every kernel that samples through these functions agrees bit for bit with the others
// and with the numpy restatement of the same order (tests/oblique_ref.py).
#pragma once
#include "pmu_common.h"

#pragma clang fp contract(off)

namespace {

struct Frame {
  double n[3], u[3], v[3];
};

__device__ __forceinline__ Frame load_frame(const double* __restrict__ f) {
  Frame r;
#pragma unroll
  for (int i = 0; i < 3; ++i) { r.n[i] = f[i]; r.u[i] = f[3 + i]; r.v[i] = f[6 + i]; }
  return r;
}

// voxel coordinate i of grid point (ds, da, db) (already scaled by h and centred)
__device__ __forceinline__ double grid_to_voxel(const Frame& f, int i, double c, double ds, double da, double db) {
  return c + ((ds * f.n[i] + da * f.u[i]) + db * f.v[i]);
}

__device__ __forceinline__ double vox_or_zero(const double* __restrict__ vol, int p0, int p1, int p2, int i, int j,
                                              int k) {
  if (i < 0 || j < 0 || k < 0 || i >= p0 || j >= p1 || k >= p2) return 0.0;
  const long long e = ((long long)i * p1 + j) * p2 + k;
  PMU_DCHECK(e >= 0 && e < (long long)p0 * p1 * p2, PMU_DBG_OPERAND);
  return vol[e];
}

// One sample of the padded volume at (x0, x1, x2).  nearest: voxel floor(x + 0.5); else trilinear,
// a + f (b - a) along axis 2, then 1, then 0.  Voxels outside the volume read as 0; a point none of
// whose corners is inside (or a NaN coordinate) is 0 without a load.
__device__ __forceinline__ double sample_volume(const double* __restrict__ vol, int p0, int p1, int p2, double x0,
                                                double x1, double x2, int nearest) {
  if (nearest) {
    const double y0 = x0 + 0.5, y1 = x1 + 0.5, y2 = x2 + 0.5;
    if (!(y0 >= 0.0 && y0 < (double)p0 && y1 >= 0.0 && y1 < (double)p1 && y2 >= 0.0 && y2 < (double)p2)) return 0.0;
    return vox_or_zero(vol, p0, p1, p2, (int)floor(y0), (int)floor(y1), (int)floor(y2));
  }
  if (!(x0 > -1.0 && x0 < (double)p0 && x1 > -1.0 && x1 < (double)p1 && x2 > -1.0 && x2 < (double)p2)) return 0.0;
  const double fl0 = floor(x0), fl1 = floor(x1), fl2 = floor(x2);
  const int i = (int)fl0, j = (int)fl1, k = (int)fl2;
  const double f0 = x0 - fl0, f1 = x1 - fl1, f2 = x2 - fl2;
  double r[2][2];
#pragma unroll
  for (int di = 0; di < 2; ++di)
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      const double a = vox_or_zero(vol, p0, p1, p2, i + di, j + dj, k);
      const double b = vox_or_zero(vol, p0, p1, p2, i + di, j + dj, k + 1);
      r[di][dj] = a + f2 * (b - a);
    }
  const double r0 = r[0][0] + f1 * (r[0][1] - r[0][0]);
  const double r1 = r[1][0] + f1 * (r[1][1] - r[1][0]);
  return r0 + f0 * (r1 - r0);
}

}  // namespace
