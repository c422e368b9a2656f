// Oblique view planes on gfx950: slices of a resident scan along any unit vector, and the fusion of
// any number of such views' predictions back onto the voxel grid.  Extends the slicer
// (PMU/utils/mri_dataset.py:60-66, whose non-standard views the reference leaves undefined) and the
// volume fusion (PMU/eval.py:157-203) beyond image[i,:,:], image[:,j,:], image[:,:,k].
//
// Geometry ("Oblique views").  A frame is nine doubles n[3] u[3] v[3] (orthonormal, made on
// the host).  The padded volume [p0][p1][p2] has centre c = (p - 1) / 2; a view samples a P x P x P grid
// of spacing h about it: slice s, pixel (a, b) sits at x = c + ((ds n + da u) + db v), d. = h (. - (P-1)/2).
// Images are sampled trilinearly in fp64 (zeros outside), masks at the nearest voxel.  The fusion maps a
// voxel back to grid coordinates g. = ((d0 f0 + d1 f1) + d2 f2) / h + (P-1)/2 and interpolates the view's
// probability stack trilinearly in fp32.  Every coordinate is evaluated in one order with FP contraction
// off (the pragma below covers the whole file), by the same device functions in every kernel (the sampler
// itself is pmu_sample.h, shared with augment.hip): the maxima and the gather agree bit for bit, and a numpy
// restatement of the same order reproduces both.
#include "pmu_common.h"
#include "pmu_sample.h"
#include "pmu_fuse.h"
#include "pmu_oblique_fuse.h"

#pragma clang fp contract(off)

namespace {

// sample e = a * P + b of slice s
__device__ __forceinline__ double sample_slice(const double* __restrict__ vol, int p0, int p1, int p2, const Frame& f,
                                               int P, double h, int s, int e, int nearest) {
  const double half = (double)(P - 1) / 2.0;
  const int a = e / P, b = e - a * P;
  const double ds = h * ((double)s - half), da = h * ((double)a - half), db = h * ((double)b - half);
  const double x0 = grid_to_voxel(f, 0, (double)(p0 - 1) / 2.0, ds, da, db);
  const double x1 = grid_to_voxel(f, 1, (double)(p1 - 1) / 2.0, ds, da, db);
  const double x2 = grid_to_voxel(f, 2, (double)(p2 - 1) / 2.0, ds, da, db);
  return sample_volume(vol, p0, p1, p2, x0, x1, x2, nearest);
}

// out[s] = max over the P*P samples of slice s (block per slice), sampled on the fly
__global__ __launch_bounds__(256) void oblique_slice_max_kernel(const double* __restrict__ vol, int p0, int p1, int p2,
                                                                const double* __restrict__ frame, int P, double h,
                                                                int nearest, double* __restrict__ out) {
  __shared__ double red[4];
  const Frame f = load_frame(frame);
  const int s = blockIdx.x;
  double m = -INFINITY;
  for (int e = threadIdx.x; e < P * P; e += blockDim.x)
    m = fmax(m, sample_slice(vol, p0, p1, p2, f, P, h, s, e, nearest));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[s] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// Item ids[b] = (scan-view row r) * P + slice.  Row r of the table: volume address vaddr[r], padded dims
// dims[r][3], frame frames[r][9]; maxv[id] the slice's max (image mode) or maxv == null.
__global__ __launch_bounds__(256) void oblique_gather_kernel(const long long* __restrict__ vaddr,
                                                             const int* __restrict__ dims,
                                                             const double* __restrict__ frames,
                                                             const double* __restrict__ maxv,
                                                             const int* __restrict__ ids, int nrows, int P, double h,
                                                             int nearest, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int id = ids[b];
  PMU_DCHECK(id >= 0 && id < nrows * P, PMU_DBG_INDEX);
  const int r = id / P, s = id - r * P;
  PMU_DCHECK(vaddr[r] != 0, PMU_DBG_INDEX);
  const double* vol = reinterpret_cast<const double*>(vaddr[r]);
  const int p0 = dims[3 * r], p1 = dims[3 * r + 1], p2 = dims[3 * r + 2];
  const Frame f = load_frame(frames + 9 * r);
  const double m = maxv ? maxv[id] : 0.0;
  const bool div = m != 0.0;
  const int px = P * P;
  float* d = out + (long long)b * px;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < px; e += gridDim.x * blockDim.x) {
    const double x = sample_slice(vol, p0, p1, p2, f, P, h, s, e, nearest);
    d[e] = div ? (float)(x / m) : (float)x;
  }
}

// ---------------- oblique fusion ----------------
// stacks [V][P][C][P][P] probabilities, frames [V][9], truth [p0][p1][p2] labels.
// A workgroup owns a row of compact BI x BJ x BK bricks along axis 2 (one voxel per thread per brick),
// so its 8 V C reads per voxel stay inside a small region of each rotated stack.  The per-view labels
// are counted per wave with ballots into that wave's LDS row (no per-thread counter arrays), summed
// over the block and leave as one exact fp64 atomic per counter per block.
constexpr int BI = 4, BJ = 8, BK = 8;
constexpr int NCNT = (FUSE_VMAX + 1) * FUSE_CMAX * 2 + FUSE_CMAX;  // (intersection, |pred|) per volume, |truth|

struct ObliqueFuseArgs {
  const float* stacks;
  const double* frames;
  const float* truth;
  int V, C, P, p0, p1, p2;
  double h;
  float* avg;
  int* label;
  int* cover;
  double* counts;
};

// (the view geometry, the coverage rule and the trilinear read: pmu_oblique_fuse.h, shared with fusion_fit.hip)
__global__ __launch_bounds__(256) void fuse_oblique_kernel(ObliqueFuseArgs a) {
  __shared__ int red[4][NCNT];
  __shared__ double fr[FUSE_VMAX][9];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int V = a.V, C = a.C, P = a.P;
  for (int e = tid; e < 4 * NCNT; e += 256) (&red[0][0])[e] = 0;
  for (int e = tid; e < 9 * V; e += 256) (&fr[0][0])[e] = a.frames[e];
  __syncthreads();
  const int i = blockIdx.y * BI + (tid >> 6);
  const int j = blockIdx.x * BJ + ((tid >> 3) & 7);
  const double d0 = (double)i - (double)(a.p0 - 1) / 2.0, d1 = (double)j - (double)(a.p1 - 1) / 2.0;
  const long long P2 = (long long)P * P, plane = (long long)a.p1 * a.p2;
  for (int k0 = 0; k0 < a.p2; k0 += BK) {
    const int k = k0 + (tid & 7);
    const bool valid = i < a.p0 && j < a.p1 && k < a.p2;
    const double d2 = (double)k - (double)(a.p2 - 1) / 2.0;
    const long long vox = ((long long)i * a.p1 + j) * a.p2 + k;
    PMU_DCHECK(!valid || (vox >= 0 && vox < (long long)a.p0 * plane), PMU_DBG_OUTPUT);
    const int t = valid ? (int)a.truth[vox] : -1;
    float sum[FUSE_CMAX];
#pragma unroll
    for (int c = 0; c < FUSE_CMAX; ++c) sum[c] = 0.f;
    int cnt = 0;
    for (int v = 0; v < V; ++v) {
      ObliqueCell q;
      const bool cov = oblique_cell(fr[v], d0, d1, d2, a.h, P, valid, q);
      int mv = 0;   // the view's label: 0 where it does not cover the voxel
      if (cov) {
        const float* st = a.stacks + (long long)v * P * C * P2;
        float best = 0.f;
        ++cnt;
#pragma unroll
        for (int c = 0; c < FUSE_CMAX; ++c) {
          if (c >= C) break;
          const float p = oblique_prob(st, q, C, c, P2);
          sum[c] += p;
          if (c == 0 || p > best) { best = p; mv = c; }
        }
      }
      for (int c = 0; c < C; ++c) {   // wave-uniform: every lane reaches the ballots
        const int np = wave_count(valid && mv == c), ni = wave_count(valid && mv == c && t == c);
        if (lane == 0) {
          red[wv][(v * FUSE_CMAX + c) * 2 + 0] += ni;
          red[wv][(v * FUSE_CMAX + c) * 2 + 1] += np;
        }
      }
    }
    // the average over the covering views (zeros where none covers), its first maximum
    int ma = 0;
    float best = 0.f;
    const float fc = (float)cnt;
#pragma unroll
    for (int c = 0; c < FUSE_CMAX; ++c) {
      if (c >= C) break;
      sum[c] = cnt ? sum[c] / fc : 0.f;
      if (c == 0 || sum[c] > best) { best = sum[c]; ma = c; }
    }
    for (int c = 0; c < C; ++c) {
      const int np = wave_count(valid && ma == c), ni = wave_count(valid && ma == c && t == c);
      const int nt = wave_count(valid && t == c);
      if (lane == 0) {
        red[wv][(V * FUSE_CMAX + c) * 2 + 0] += ni;
        red[wv][(V * FUSE_CMAX + c) * 2 + 1] += np;
        red[wv][(FUSE_VMAX + 1) * FUSE_CMAX * 2 + c] += nt;
      }
    }
    if (valid) {
      if (a.avg) {
#pragma unroll
        for (int c = 0; c < FUSE_CMAX; ++c)
          if (c < C) a.avg[((long long)i * C + c) * plane + (long long)j * a.p2 + k] = sum[c];
      }
      if (a.label) a.label[vox] = ma;
      if (a.cover) a.cover[vox] = cnt;
    }
  }
  __syncthreads();
  // counts[(V+1)][C][3]: one atomic per non-zero counter per block (integers in fp64: exact)
  if (tid < (V + 1) * C * 3) {
    const int w = tid / (3 * C), rem = tid - w * 3 * C, c = rem / 3, q = rem - c * 3;
    const int slot = (q == 2) ? (FUSE_VMAX + 1) * FUSE_CMAX * 2 + c : (w * FUSE_CMAX + c) * 2 + q;
    const int x = red[0][slot] + red[1][slot] + red[2][slot] + red[3][slot];
    if (x) atomicAdd(a.counts + (w * C + c) * 3 + q, (double)x);
  }
}

}  // namespace

extern "C" int pmu_oblique_slice_max(const double* vol, int p0, int p1, int p2, const double* frame, int P, double h,
                                     int nearest, double* out, void* stream) {
  PMU_REQUIRE(vol && frame && out && p0 > 0 && p1 > 0 && p2 > 0 && P >= 2 && P <= 32768 && h > 0.0);
  hipLaunchKernelGGL(oblique_slice_max_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, vol, p0, p1, p2,
                     frame, P, h, nearest, out);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_oblique_gather(const long long* vaddr, const int* dims, const double* frames, const double* maxv,
                                  const int* ids, int B, int nrows, int P, double h, int nearest, float* out,
                                  void* stream) {
  PMU_REQUIRE(vaddr && dims && frames && ids && out && B > 0 && B <= 65535 && nrows > 0 && P >= 2 && P <= 32768 &&
              (long long)nrows * P < (1LL << 31) && h > 0.0);
  int gx = pmu_cdiv((long long)P * P, 256);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(oblique_gather_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, vaddr,
                     dims, frames, maxv, ids, nrows, P, h, nearest, out);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_fuse_oblique(const float* stacks, const double* frames, int V, int C, int P, double h,
                                const float* truth, int p0, int p1, int p2, float* avg, int* label, int* cover,
                                double* counts, void* stream) {
  PMU_REQUIRE(stacks && frames && truth && counts && V >= 1 && V <= FUSE_VMAX && C >= 1 && C <= FUSE_CMAX && P >= 2 &&
              P <= 32768 && h > 0.0 && p0 > 0 && p1 > 0 && p2 > 0);
  PMU_REQUIRE(pmu_cdiv(p0, BI) <= 65535);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(double) * (V + 1) * C * 3, st) != hipSuccess) return PMU_ERR_ARG;
  ObliqueFuseArgs a{stacks, frames, truth, V, C, P, p0, p1, p2, h, avg, label, cover, counts};
  hipLaunchKernelGGL(fuse_oblique_kernel, dim3((unsigned)pmu_cdiv(p1, BJ), (unsigned)pmu_cdiv(p0, BI)), dim3(256), 0,
                     st, a);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
