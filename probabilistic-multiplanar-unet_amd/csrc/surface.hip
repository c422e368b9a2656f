// Surface-distance kernels: the exact squared Euclidean distance transform to a class surface
// (pmu_surface_edt) and the gather of one volume's surface distances from another's transform
// (pmu_surface_collect).  pmu_hip/surface.py builds HD / HD95 / ASSD / surface Dice on them.  pmu_interior_edt is
// the same transform seeded from outside the class (every voxel not labelled cls, and the positions outside the
// volume), 0 off the class: the field the covering pass of thickness.hip starts from.
//
// lab u8 [D0][D1][D2].  The surface of class c: every voxel labelled c with one of its six face neighbours not
// labelled c, a neighbour outside the volume counting as not c (mask ^ binary_erosion(mask), 6-connected,
// border value 0).  Under fp32 voxel sizes (s0, s1, s2) the squared distance of an index difference is
//     t_i = fl(fl(s_i * float(d_i)) * fl(s_i * float(d_i))),    d2 = fl(fl(t_2 + t_1) + t_0),
// every operation a single rounding (__fmul_rn / __fadd_rn and FP contraction off for the file), so the
// numpy restatement tests/surface_ref.py computes the same bits.
//
// The transform is separable, axis 2 (contiguous), then axis 1, then axis 0, each pass
// g(j) = min_k fl(f(k) + t(j - k)).  fp32 addition of a fixed non-negative term is monotone, so the
// minimum of a pass commutes with the next pass's addition and the result is bit-equal to the brute-force
// minimum of d2 over all surface voxels.
//   pass 2  surface_row_kernel: four rows per 256-thread block.  A wave reduces 64 voxels of a row to one
//           ballot word of surface bits in LDS (no mask in memory); in one dimension the minimum is the t
//           of the nearest set bit, found by clz / ctz over the row's at most 16 words.  The surface count
//           is one integer atomicAdd per wave.
//   pass 1, pass 0  column_pass_kernel on lines of length L with stride N: a block stages a tile of W
//           contiguous voxels by the whole line in LDS (global reads and writes stay coalesced), with the
//           table t(0..L-1); each thread scans k outward from j and stops at the first t(d) >= best — exact
//           pruning, since t is non-decreasing in d and fl(f + t) >= t for f >= 0.  In place: a block reads
//           and writes only its own lines.  The scan costs about 2 sqrt(d2) / s LDS reads per voxel, which
//           is what keeps the transform far above its bytes bound on a volume whose voxels lie tens of voxels
//           from the surface (DESIGN.md "Surface distances").
#include "pmu_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SF_MAXDIM = PMU_SURFACE_MAX_DIM;
constexpr int SF_ROWS = 4;                    // rows of one surface_row_kernel block
constexpr int SF_WORDS = SF_MAXDIM / 64;      // ballot words of the longest row
constexpr int SF_TILE = 16384;                // floats of a column tile: 64 KiB, two blocks per CU with the table
constexpr int SF_CT = 512;                    // threads of a column_pass_kernel block
static_assert(2 * (SF_TILE + SF_MAXDIM) * 4 <= 160 * 1024, "two column tiles and tables fit the LDS of a CU");
static_assert(SF_TILE / SF_MAXDIM >= 1, "the longest line fits the tile");

__device__ __forceinline__ float sq_step(float s, int d) {
  const float a = __fmul_rn(s, (float)d);
  return __fmul_rn(a, a);
}

// voxel v = (i0, i1, i2) is on the surface of class cls
__device__ __forceinline__ bool on_surface(const unsigned char* __restrict__ lab, int D0, int D1, int D2, int i0,
                                           int i1, int i2, long long v, unsigned cls) {
  PMU_DCHECK(i0 >= 0 && i0 < D0 && i1 >= 0 && i1 < D1 && i2 >= 0 && i2 < D2 &&
                 v == ((long long)i0 * D1 + i1) * D2 + i2,
             PMU_DBG_OPERAND);
  if (lab[v] != cls) return false;
  const long long s1 = D2, s0 = (long long)D1 * D2;
  bool inside = i2 > 0 && i2 < D2 - 1 && i1 > 0 && i1 < D1 - 1 && i0 > 0 && i0 < D0 - 1;
  if (inside)
    inside = lab[v - 1] == cls && lab[v + 1] == cls && lab[v - s1] == cls && lab[v + s1] == cls &&
             lab[v - s0] == cls && lab[v + s0] == cls;
  return !inside;
}

// INTERIOR = false: the seeds of a row are its surface voxels, and they are counted (pmu_surface_edt).
// INTERIOR = true: the seeds are the voxels not labelled cls, and the voxels labelled cls are counted
// (pmu_interior_edt).  Everything else is shared.
template <bool INTERIOR>
__global__ __launch_bounds__(256) void surface_row_kernel(const unsigned char* __restrict__ lab, int D0, int D1,
                                                          int D2, unsigned cls, float s2, float* __restrict__ d2,
                                                          unsigned long long* __restrict__ n_surface) {
  __shared__ unsigned long long masks[SF_ROWS][SF_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cw = (D2 + 63) >> 6;  // ballot words of a row
  const long long rows = (long long)D0 * D1;
  const long long row0 = (long long)blockIdx.x * SF_ROWS;
  PMU_DCHECK(row0 < rows && cw <= SF_WORDS, PMU_DBG_GRID);
  unsigned long long count = 0;
  for (int c = wave; c < SF_ROWS * cw; c += 4) {  // wave-uniform
    const int rr = c / cw, word = c - rr * cw;
    const long long r = row0 + rr;
    const int j = word * 64 + lane;
    bool s = false;
    if (r < rows && j < D2) {
      if constexpr (INTERIOR) {
        PMU_DCHECK(r * D2 + j < rows * D2, PMU_DBG_OPERAND);
        s = lab[r * D2 + j] != cls;
      } else {
        const int i0 = (int)(r / D1), i1 = (int)(r - (long long)i0 * D1);
        s = on_surface(lab, D0, D1, D2, i0, i1, j, r * D2 + j, cls);
      }
    }
    const unsigned long long m = __ballot(s);
    if (lane == 0) masks[rr][word] = m;
    if constexpr (INTERIOR)
      count += (unsigned long long)__popcll(__ballot(r < rows && j < D2 && !s));
    else
      count += (unsigned long long)__popcll(m);
  }
  if (lane == 0 && count) atomicAdd(n_surface, count);
  __syncthreads();
  for (int c = wave; c < SF_ROWS * cw; c += 4) {
    const int rr = c / cw, word = c - rr * cw;
    const long long r = row0 + rr;
    const int j = word * 64 + lane;
    if (r >= rows || j >= D2) continue;
    int dist = -1;  // index distance to the nearest surface voxel of the row; -1: none
    const unsigned long long upto = ~0ull >> (63 - lane);  // bits <= lane
    unsigned long long m = masks[rr][word] & upto;
    for (int w = word;;) {
      if (m) {
        dist = j - (w * 64 + 63 - __builtin_clzll(m));
        break;
      }
      if (--w < 0) break;
      m = masks[rr][w];
    }
    m = masks[rr][word] & ~upto;
    for (int w = word;;) {
      if (m) {
        const int d = w * 64 + __builtin_ctzll(m) - j;
        if (dist < 0 || d < dist) dist = d;
        break;
      }
      if (++w >= cw) break;
      m = masks[rr][w];
    }
    PMU_DCHECK(dist < D2, PMU_DBG_INDEX);
    PMU_DCHECK(r * D2 + j < rows * D2, PMU_DBG_OUTPUT);
    d2[r * D2 + j] = dist < 0 ? __builtin_inff() : sq_step(s2, dist);
  }
}

// One pass over lines of length L: element (o, j, p) at d2[(o * L + j) * N + p], o < nouter, p < N.  Block b owns
// outer index o = b / tiles and the columns p0 = (b % tiles) * W .. p0 + W of it (tiles = ceil(N / W),
// L * W <= SF_TILE, W <= 64, W % V == 0).  A thread scans V adjacent columns of one j at a time (V = 4: one
// ds_read_b128 per side and step instead of four ds_read_b32; LDS reads bound this kernel), until no column of
// its own can improve.  Columns without a finite value (no surface in their line so far: about half the lines
// of the axis-1 pass on a volume whose structures span half of axis 0) stay +inf and are not scanned.
template <int V>
__device__ __forceinline__ void ld_cols(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__global__ __launch_bounds__(SF_CT) void column_pass_kernel(float* __restrict__ d2, int nouter, int L, long long N,
                                                            int W, int tiles, float s) {
  __shared__ __attribute__((aligned(16))) float tile[SF_TILE];
  __shared__ float tab[SF_MAXDIM];
  __shared__ int colfin[64];  // column x of the tile holds a finite value
  const int tid = threadIdx.x;
  const int o = (int)(blockIdx.x / (unsigned)tiles);
  const long long p0 = (long long)(blockIdx.x - (unsigned)o * (unsigned)tiles) * W;
  PMU_DCHECK(o < nouter && p0 < N && L <= SF_MAXDIM && (long long)L * W <= SF_TILE && W <= 64 && W % V == 0,
             PMU_DBG_GRID);
  const int wt = (int)(N - p0 < W ? N - p0 : W);  // columns of this tile
  float* base = d2 + (long long)o * L * N + p0;
  const int elems = L * W;
  const float inf = __builtin_inff();
  for (int d = tid; d < L; d += SF_CT) tab[d] = sq_step(s, d);
  if (tid < 64) colfin[tid] = 0;
  __syncthreads();
  for (int e = tid; e < elems; e += SF_CT) {
    const int j = e / W, x = e - j * W;
    float v = inf;  // columns past the volume: never scanned, never stored
    if (x < wt) {
      PMU_DCHECK(((long long)o * L + j) * N + p0 + x < (long long)nouter * L * N, PMU_DBG_OPERAND);
      v = base[(long long)j * N + x];
    }
    tile[e] = v;
    if (v < inf) colfin[x] = 1;  // (every writer stores the same value)
  }
  __syncthreads();
  const int wv = W / V;
  const int items = L * wv;
  for (int i = tid; i < items; i += SF_CT) {
    const int j = i / wv, x = (i - j * wv) * V;
    const int e = j * W + x;
    float b[V];
    bool fin[V];
    bool any = false;
    ld_cols<V>(tile + e, b);
#pragma unroll
    for (int c = 0; c < V; ++c) {
      fin[c] = colfin[x + c] != 0;
      any = any || fin[c];
    }
    if (any) {
      const int up = j, dn = L - 1 - j;
      const int far = up > dn ? up : dn;
      for (int d = 1; d <= far; ++d) {
        const float t = tab[d];
        bool go = false;  // fl(f + t) >= t: past t >= best no farther voxel can improve a column
#pragma unroll
        for (int c = 0; c < V; ++c) go = go || (fin[c] && t < b[c]);
        if (!go) break;
        float q[V];
        if (d <= up) {
          ld_cols<V>(tile + e - d * W, q);
#pragma unroll
          for (int c = 0; c < V; ++c) b[c] = fminf(b[c], __fadd_rn(q[c], t));
        }
        if (d <= dn) {
          ld_cols<V>(tile + e + d * W, q);
#pragma unroll
          for (int c = 0; c < V; ++c) b[c] = fminf(b[c], __fadd_rn(q[c], t));
        }
      }
    }
#pragma unroll
    for (int c = 0; c < V; ++c)
      if (x + c < wt) {
        PMU_DCHECK(((long long)o * L + j) * N + p0 + x + c < (long long)nouter * L * N, PMU_DBG_OUTPUT);
        base[(long long)j * N + x + c] = b[c];
      }
  }
}

__global__ __launch_bounds__(256) void surface_collect_kernel(const unsigned char* __restrict__ lab, int D0, int D1,
                                                              int D2, unsigned cls,
                                                              const float* __restrict__ d2_other,
                                                              float* __restrict__ out, long long cap,
                                                              unsigned long long* __restrict__ n_out) {
  const long long total = (long long)D0 * D1 * D2;
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * 256;
  for (long long b = (long long)blockIdx.x * 256; b < total; b += stride) {  // block-uniform trip count
    const long long v = b + threadIdx.x;
    bool s = false;
    if (v < total) {
      const long long r = v / D2;
      const int i2 = (int)(v - r * D2), i0 = (int)(r / D1), i1 = (int)(r - (long long)i0 * D1);
      s = on_surface(lab, D0, D1, D2, i0, i1, i2, v, cls);
    }
    const unsigned long long m = __ballot(s);
    if (!m) continue;  // wave-uniform
    unsigned long long slot0 = 0;
    if (lane == 0) slot0 = atomicAdd(n_out, (unsigned long long)__popcll(m));
    slot0 = __shfl(slot0, 0, 64);
    if (s) {
      const unsigned long long slot = slot0 + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
      PMU_DCHECK(slot < (unsigned long long)total, PMU_DBG_INDEX);
      if (slot < (unsigned long long)cap) out[slot] = d2_other[v];
    }
  }
}

// The border term of the interior distance: a position outside the volume is not of the class, and the nearest
// one lies straight out along one axis, min(i + 1, D - i) voxels away.  One thread per voxel, after the passes
// (the term of an axis cannot enter before that axis's pass: the pass would add to it).
__global__ __launch_bounds__(256) void interior_border_kernel(float* __restrict__ d2, int D0, int D1, int D2,
                                                              float s0, float s1, float s2) {
  const long long total = (long long)D0 * D1 * D2;
  const long long stride = (long long)gridDim.x * 256;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += stride) {
    const float f = d2[v];
    if (f == 0.f) continue;  // not of the class: nothing is nearer than the voxel itself
    const long long r = v / D2;
    const int i2 = (int)(v - r * D2), i0 = (int)(r / D1), i1 = (int)(r - (long long)i0 * D1);
    const int o2 = i2 + 1 < D2 - i2 ? i2 + 1 : D2 - i2;
    const int o1 = i1 + 1 < D1 - i1 ? i1 + 1 : D1 - i1;
    const int o0 = i0 + 1 < D0 - i0 ? i0 + 1 : D0 - i0;
    const float b = fminf(fminf(sq_step(s2, o2), sq_step(s1, o1)), sq_step(s0, o0));
    if (b < f) d2[v] = b;
  }
}

bool volume_ok(int D0, int D1, int D2, int cls) {
  if (D0 < 1 || D0 > SF_MAXDIM || D1 < 1 || D1 > SF_MAXDIM || D2 < 1 || D2 > SF_MAXDIM) return false;
  if ((long long)D0 * D1 * D2 >= (1LL << 31)) return false;
  return cls >= 0 && cls <= 255;
}
bool spacing_ok(float s) { return s > 0.f && s <= 3.402823466e38f; }  // finite and positive (NaN fails both)

int column_pass(float* d2, int nouter, int L, long long N, float s, hipStream_t st) {
  if (L == 1) return PMU_OK;  // g = f
  long long W = SF_TILE / L;  // >= 16
  if (W > 64) W = 64;
  if (W > N) W = N;
  const bool vec = W >= 4;       // four columns per thread; fewer than four only in a volume that narrow
  if (vec) W &= ~3LL;
  const long long tiles = (N + W - 1) / W;
  const long long blocks = tiles * nouter;
  PMU_REQUIRE(blocks >= 1 && blocks < (1LL << 31));
  if (vec)
    hipLaunchKernelGGL(column_pass_kernel<4>, dim3((unsigned)blocks), dim3(SF_CT), 0, st, d2, nouter, L, N, (int)W,
                       (int)tiles, s);
  else
    hipLaunchKernelGGL(column_pass_kernel<1>, dim3((unsigned)blocks), dim3(SF_CT), 0, st, d2, nouter, L, N, (int)W,
                       (int)tiles, s);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

}  // namespace

extern "C" int pmu_surface_edt(const unsigned char* lab, int D0, int D1, int D2, int cls, float s0, float s1,
                               float s2, float* d2, unsigned long long* n_surface, void* stream) {
  PMU_REQUIRE(lab && d2 && n_surface && volume_ok(D0, D1, D2, cls));
  PMU_REQUIRE(spacing_ok(s0) && spacing_ok(s1) && spacing_ok(s2));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(n_surface, 0, sizeof(unsigned long long), st) != hipSuccess) return PMU_ERR_ARG;
  const long long rows = (long long)D0 * D1;
  hipLaunchKernelGGL(surface_row_kernel<false>, dim3((unsigned)((rows + SF_ROWS - 1) / SF_ROWS)), dim3(256), 0, st,
                     lab, D0, D1, D2, (unsigned)cls, s2, d2, n_surface);
  PMU_CHECK_LAUNCH();
  int rc = column_pass(d2, D0, D1, D2, s1, st);
  if (rc) return rc;
  return column_pass(d2, 1, D0, (long long)D1 * D2, s0, st);
}

extern "C" int pmu_interior_edt(const unsigned char* lab, int D0, int D1, int D2, int cls, float s0, float s1,
                                float s2, float* d2, unsigned long long* n_voxels, void* stream) {
  PMU_REQUIRE(lab && d2 && n_voxels && volume_ok(D0, D1, D2, cls));
  PMU_REQUIRE(spacing_ok(s0) && spacing_ok(s1) && spacing_ok(s2));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(n_voxels, 0, sizeof(unsigned long long), st) != hipSuccess) return PMU_ERR_ARG;
  const long long rows = (long long)D0 * D1;
  hipLaunchKernelGGL(surface_row_kernel<true>, dim3((unsigned)((rows + SF_ROWS - 1) / SF_ROWS)), dim3(256), 0, st,
                     lab, D0, D1, D2, (unsigned)cls, s2, d2, n_voxels);
  PMU_CHECK_LAUNCH();
  int rc = column_pass(d2, D0, D1, D2, s1, st);
  if (rc) return rc;
  rc = column_pass(d2, 1, D0, (long long)D1 * D2, s0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(interior_border_kernel, dim3(grid_for((long long)D0 * D1 * D2)), dim3(256), 0, st, d2, D0, D1, D2,
                     s0, s1, s2);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_surface_collect(const unsigned char* lab, int D0, int D1, int D2, int cls, const float* d2_other,
                                   float* out, long long cap, unsigned long long* n_out, void* stream) {
  PMU_REQUIRE(lab && d2_other && n_out && volume_ok(D0, D1, D2, cls) && cap >= 0 && (out || cap == 0));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(n_out, 0, sizeof(unsigned long long), st) != hipSuccess) return PMU_ERR_ARG;
  hipLaunchKernelGGL(surface_collect_kernel, dim3(grid_for((long long)D0 * D1 * D2)), dim3(256), 0, st, lab, D0, D1,
                     D2, (unsigned)cls, d2_other, out, cap, n_out);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
