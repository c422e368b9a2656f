// 3-D connected components of a label volume (pmu_cc_label), their dense numbering (pmu_cc_compact), sizes and
// classes (pmu_cc_sizes), the filter that keeps a chosen set (pmu_cc_filter) and the component-to-class overlap
// test of two volumes (pmu_cc_overlap).  pmu_hip/components.py builds keep_largest and the lesion-wise detection
// scores on them.
//
// lab u8 [D0][D1][D2], V voxels, value 0 = background.  Two voxels are adjacent when their index difference has
// every component in {-1, 0, 1} and at most 1 (connectivity 6), 2 (18) or 3 (26) non-zero components; a component
// is a maximal set of voxels of one non-zero value joined by chains of adjacent voxels.  root[v] = 1 + the
// smallest linear index of v's component (0 for background): a canonical map, independent of the order in which
// anything ran, which tests/components_ref.py restates in numpy bit for bit.
//
// pmu_cc_label is a label-equivalence union-find whose forest lives in root itself (entry v holds 1 + the index
// of v's parent, a root holds 1 + its own index; a parent's index never exceeds the child's, so there are no
// cycles and the root of a finished tree is the component's smallest index).  Three launches, whatever the data:
//   cc_local_kernel    one 256-thread block per CC_T0 x CC_T1 x CC_T2 tile: the tile's labels and a parent
//                      array of local indices in LDS.  A voxel starts at the first voxel of its run along
//                      axis 2 (a wave holds one row: a ballot), then one union (LDS atomicMin) per voxel and
//                      other backward neighbour inside the tile, skipped where the pair one step to the left
//                      joins the same two runs; then every voxel of the tile is written pointing at its tile
//                      root.  Local index order is linear index order, so the tile root is the tile minimum.
//   cc_merge_kernel    one thread per voxel on a tile border: a union in global memory for every backward
//                      neighbour of the same value in another tile.  The forest is read and written through
//                      relaxed agent-scope atomics only (a plain load may be served from a stale line of another
//                      XCD's L2 or the CU's L1).  union_global retries from the value atomicMin returns when the
//                      larger root had stopped being one; parent values only decrease, so the loop ends whatever
//                      other workgroups do, and nothing ever waits for another workgroup.
//   cc_flatten_kernel  every voxel follows its chain to the root and stores it; a voxel that is its own root is
//                      counted (ballot, one integer atomicAdd per wave at the end of a grid-stride loop).
//                      Concurrent stores only replace an ancestor by the root: any value a reader meets leads to
//                      the same root.
// pmu_cc_compact ranks the roots in ascending order (scipy.ndimage.label's numbering) by reduce-then-scan over
// the flags root[v] == v + 1: per-block counts, one single-block scan of them, then two passes in place — roots
// take the negative of their rank (cc_mark_kernel), then every voxel takes |ids[root - 1]| (cc_resolve_kernel;
// the entry of a root is -rank or +rank at any moment of that launch, so the result does not depend on order).
// That split is what lets ids alias root.
#include "pmu_common.h"

namespace {

constexpr int CC_MAXDIM = PMU_CC_MAX_DIM;
constexpr int CC_T0 = 4, CC_T1 = 8, CC_T2 = 64;      // tile of one cc_local_kernel block
constexpr int CC_TV = CC_T0 * CC_T1 * CC_T2;          // 2048 voxels: 8 KiB of parents + 2 KiB of labels in LDS
constexpr int CC_THREADS = 256;
constexpr int CC_CHUNK = 2048;                        // voxels of one compact block (8 per thread)
constexpr int CC_SCAN_THREADS = 1024;
constexpr int CC_SIZE_STEPS = 16;                    // 64-voxel steps of one wave of cc_sizes_kernel
static_assert(CC_TV % CC_THREADS == 0 && CC_CHUNK % CC_THREADS == 0, "whole voxels per thread");
static_assert(CC_T2 == 64 && CC_THREADS % 64 == 0, "a wave of cc_local_kernel holds one row of the tile");

// The 13 backward neighbours (first non-zero component negative), by number of non-zero components.
__constant__ signed char cc_off[13][4] = {
    {0, 0, -1, 1},  {0, -1, 0, 1},  {-1, 0, 0, 1},                                               // faces
    {0, -1, -1, 2}, {0, -1, 1, 2},  {-1, 0, -1, 2}, {-1, 0, 1, 2}, {-1, -1, 0, 2}, {-1, 1, 0, 2},  // edges
    {-1, -1, -1, 3}, {-1, -1, 1, 3}, {-1, 1, -1, 3}, {-1, 1, 1, 3}};                              // corners

__device__ __forceinline__ int lds_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int agent_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void agent_store(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS forest of local indices: par[x] == x at a root.
__device__ __forceinline__ int find_local(const int* par, int x) {
  for (;;) {
    PMU_DCHECK(x >= 0 && x < CC_TV, PMU_DBG_INDEX);
    const int p = lds_load(par + x);
    if (p == x) return x;
    x = p;  // p < x
  }
}
__device__ __forceinline__ void union_local(int* par, int a, int b) {
  a = find_local(par, a);
  b = find_local(par, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(par + a, b);  // a > b
    if (old == a) break;                    // a was a root and now hangs under b
    a = find_local(par, old);               // a had a parent already (old < a): join that tree with b's
    b = find_local(par, b);
  }
}

// Global forest in root: entry x holds 1 + parent index, 1 + x at a root.  Indices here are 0-based.
__device__ __forceinline__ int find_global(const int* P, int x, int V) {
  for (;;) {
    PMU_DCHECK(x >= 0 && x < V, PMU_DBG_INDEX);
    const int p = agent_load(P + x) - 1;
    if (p == x) return x;
    PMU_DCHECK(p >= 0 && p < x, PMU_DBG_INDEX);
    x = p;
  }
}
__device__ __forceinline__ void union_global(int* P, int a, int b, int V) {
  a = find_global(P, a, V);
  b = find_global(P, b, V);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b + 1) - 1;  // a > b; (agent scope, relaxed)
    if (old == a) break;
    a = find_global(P, old, V);  // the values only decrease: this loop ends
    b = find_global(P, b, V);
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const unsigned char* __restrict__ lab, int D0, int D1,
                                                              int D2, int maxnz, int tiles1, int tiles2,
                                                              int* __restrict__ P) {
  __shared__ int par[CC_TV];
  __shared__ unsigned char sl[CC_TV];
  const int tid = threadIdx.x;
  const int b2 = (int)(blockIdx.x % (unsigned)tiles2);
  const int b01 = (int)(blockIdx.x / (unsigned)tiles2);
  const int b1 = b01 % tiles1, b0 = b01 / tiles1;
  const int z0 = b0 * CC_T0, y0 = b1 * CC_T1, x0 = b2 * CC_T2;
  PMU_DCHECK(z0 < D0 && y0 < D1 && x0 < D2, PMU_DBG_GRID);
  for (int l = tid; l < CC_TV; l += CC_THREADS) {
    const int lx = l % CC_T2, ly = (l / CC_T2) % CC_T1, lz = l / (CC_T2 * CC_T1);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    unsigned char c = 0;  // outside the volume: background
    if (z < D0 && y < D1 && x < D2) c = lab[((long long)z * D1 + y) * D2 + x];
    sl[l] = c;
    // A wave holds one row of the tile (lane = lx): every voxel starts at the first voxel of its run along x,
    // which is all the (0, 0, -1) neighbour has to contribute.
    const int left = __shfl_up((int)c, 1, 64);
    const unsigned long long starts = __ballot(c != 0 && (lx == 0 || left != (int)c));
    int p = l;
    if (c) p = l - lx + (63 - __builtin_clzll(starts & (~0ull >> (63 - lx))));
    PMU_DCHECK(p >= l - lx && p <= l, PMU_DBG_INDEX);
    par[l] = p;
  }
  __syncthreads();
  for (int l = tid; l < CC_TV; l += CC_THREADS) {
    const unsigned char c = sl[l];
    if (!c) continue;
    const int lx = l % CC_T2, ly = (l / CC_T2) % CC_T1, lz = l / (CC_T2 * CC_T1);
    for (int k = 1; k < 13; ++k) {  // (k = 0 is the run along x)
      if (cc_off[k][3] > maxnz) break;
      const int nz = lz + cc_off[k][0], ny = ly + cc_off[k][1], nx = lx + cc_off[k][2];
      if (nz < 0 || ny < 0 || ny >= CC_T1 || nx < 0 || nx >= CC_T2) continue;
      const int nl = (nz * CC_T1 + ny) * CC_T2 + nx;
      PMU_DCHECK(nl >= 0 && nl < l, PMU_DBG_INDEX);
      if (sl[nl] != c) continue;
      // the pair one step to the left has the same offset, and each of its voxels shares a run with ours: it
      // joins the same two runs (or is itself skipped for the pair left of it, down to one that is not)
      if (lx > 0 && nx > 0 && sl[l - 1] == c && sl[nl - 1] == c) continue;
      union_local(par, l, nl);
    }
  }
  __syncthreads();
  for (int l = tid; l < CC_TV; l += CC_THREADS) {
    const int lx = l % CC_T2, ly = (l / CC_T2) % CC_T1, lz = l / (CC_T2 * CC_T1);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    if (z >= D0 || y >= D1 || x >= D2) continue;
    int out = 0;
    if (sl[l]) {
      const int r = find_local(par, l);  // (nothing writes par any more)
      const int rx = r % CC_T2, ry = (r / CC_T2) % CC_T1, rz = r / (CC_T2 * CC_T1);
      PMU_DCHECK(z0 + rz < D0 && y0 + ry < D1 && x0 + rx < D2 && sl[r] == sl[l], PMU_DBG_INDEX);
      out = ((z0 + rz) * D1 + (y0 + ry)) * D2 + (x0 + rx) + 1;  // < 2^31: V < 2^31
    }
    PMU_DCHECK(((long long)z * D1 + y) * D2 + x < (long long)D0 * D1 * D2, PMU_DBG_OUTPUT);
    P[((long long)z * D1 + y) * D2 + x] = out;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const unsigned char* __restrict__ lab, int D0, int D1,
                                                              int D2, int maxnz, int* P) {
  const int V = D0 * D1 * D2;
  const long long vv = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (vv >= V) return;
  const int v = (int)vv;
  const int x = v % D2, r = v / D2, y = r % D1, z = r / D1;
  const int lx = x % CC_T2, ly = y % CC_T1, lz = z % CC_T0;
  // only a voxel on these faces of its tile has a backward neighbour in another tile
  if (!(lz == 0 || ly == 0 || ly == CC_T1 - 1 || lx == 0 || lx == CC_T2 - 1)) return;
  const unsigned char c = lab[v];
  if (!c) return;
  for (int k = 0; k < 13; ++k) {
    if (cc_off[k][3] > maxnz) break;
    const int dz = cc_off[k][0], dy = cc_off[k][1], dx = cc_off[k][2];
    const bool same_tile = lz + dz >= 0 && ly + dy >= 0 && ly + dy < CC_T1 && lx + dx >= 0 && lx + dx < CC_T2;
    if (same_tile) continue;  // joined by cc_local_kernel
    const int nz = z + dz, ny = y + dy, nx = x + dx;
    if (nz < 0 || ny < 0 || ny >= D1 || nx < 0 || nx >= D2) continue;
    const int nv = (nz * D1 + ny) * D2 + nx;
    PMU_DCHECK(nv >= 0 && nv < v, PMU_DBG_OPERAND);
    if (lab[nv] != c) continue;
    // as in cc_local_kernel: the pair one step to the left crosses the same tile face and joins the same two
    // runs, when both left voxels lie in the tiles of v and nv and carry the value
    if (lx > 0 && nx % CC_T2 > 0 && lab[v - 1] == c && lab[nv - 1] == c) continue;
    union_global(P, v, nv, V);
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* P, int V,
                                                                unsigned long long* __restrict__ n_components) {
  const long long stride = (long long)gridDim.x * CC_THREADS;
  unsigned long long count = 0;
  for (long long b = (long long)blockIdx.x * CC_THREADS; b < V; b += stride) {  // block-uniform trip count
    const long long v = b + threadIdx.x;
    bool is_root = false;
    if (v < V && agent_load(P + v) != 0) {
      const int r = find_global(P, (int)v, V);
      is_root = r == (int)v;
      if (!is_root) agent_store(P + v, r + 1);
    }
    count += (unsigned long long)__popcll(__ballot(is_root));
  }
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(n_components, count);
}

__device__ __forceinline__ bool root_flag(const int* root, long long v) { return root[v] == (int)(v + 1); }

// block sum of one int per thread (CC_THREADS threads), returned to every thread
__device__ __forceinline__ int block_sum(int x, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < CC_THREADS / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int* __restrict__ root, long long V,
                                                              unsigned* __restrict__ counts) {
  __shared__ int red[CC_THREADS / 64];
  const long long base = (long long)blockIdx.x * CC_CHUNK;
  int c = 0;
  for (int e = threadIdx.x; e < CC_CHUNK; e += CC_THREADS) {
    const long long v = base + e;
    if (v < V) c += root_flag(root, v);
  }
  c = block_sum(c, red);
  if (threadIdx.x == 0) counts[blockIdx.x] = (unsigned)c;
}

// One block: counts[0..nb) -> exclusive prefix sums in place, *n = the total.
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_scan_kernel(unsigned* __restrict__ counts, long long nb,
                                                                  unsigned long long* __restrict__ n) {
  __shared__ unsigned wsum[CC_SCAN_THREADS / 64];
  __shared__ unsigned carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0u;
  __syncthreads();
  for (long long b0 = 0; b0 < nb; b0 += CC_SCAN_THREADS) {  // block-uniform
    const long long i = b0 + tid;
    const unsigned x = i < nb ? counts[i] : 0u;
    unsigned inc = x;  // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (i < nb) counts[i] = before + inc - x;
    __syncthreads();  // carry_s and wsum are read
    if (tid == CC_SCAN_THREADS - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (tid == 0) *n = (unsigned long long)carry_s;
}

__global__ __launch_bounds__(CC_THREADS) void cc_mark_kernel(const int* root, long long V,
                                                             const unsigned* __restrict__ offsets, int* ids) {
  __shared__ int wpre[CC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = (long long)blockIdx.x * CC_CHUNK;
  int before = (int)offsets[blockIdx.x];  // roots before this step of the chunk
  for (int e0 = 0; e0 < CC_CHUNK; e0 += CC_THREADS) {  // block-uniform
    const long long v = base + e0 + tid;
    int val = 0;
    bool f = false;
    if (v < V) {
      val = root[v];
      f = val == (int)(v + 1);
    }
    const unsigned long long m = __ballot(f);
    __syncthreads();  // the previous step's wpre is read
    if (lane == 0) wpre[wave] = __popcll(m);
    __syncthreads();
    int pre = before;
    for (int w = 0; w < wave; ++w) pre += wpre[w];
    int tot = 0;
#pragma unroll
    for (int w = 0; w < CC_THREADS / 64; ++w) tot += wpre[w];
    if (v < V) {
      const int rank = pre + __popcll(m & ((1ull << lane) - 1ull)) + 1;
      PMU_DCHECK(rank >= 1 && (long long)rank <= V, PMU_DBG_INDEX);
      ids[v] = f ? -rank : val;
    }
    before += tot;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_resolve_kernel(int* ids, long long V) {
  const long long stride = (long long)gridDim.x * CC_THREADS;
  for (long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x; v < V; v += stride) {
    const int x = agent_load(ids + v);
    if (x == 0) continue;
    int rank;
    if (x < 0) {
      rank = -x;  // a root
    } else {
      PMU_DCHECK((long long)x <= V, PMU_DBG_INDEX);
      if ((long long)x > V) continue;  // not a root map: leave the entry
      const int y = agent_load(ids + (x - 1));  // the root's entry: -rank, or +rank once its own thread ran
      PMU_DCHECK(y != 0, PMU_DBG_INDEX);
      rank = y < 0 ? -y : y;
    }
    agent_store(ids + v, rank);
  }
}

// A wave walks CC_SIZE_STEPS steps of 64 consecutive voxels.  The voxels of a step fall into runs of one id: the
// first lane of a run adds the run's length; a step that is one run of the id carried from the steps before only
// lengthens the carry, which is added when the id changes (one atomic per 1024 voxels inside a large component).
__global__ __launch_bounds__(CC_THREADS) void cc_sizes_kernel(const int* __restrict__ ids,
                                                              const unsigned char* __restrict__ lab, long long V,
                                                              long long n, unsigned long long* __restrict__ size,
                                                              unsigned char* __restrict__ cls) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = ((long long)blockIdx.x * (CC_THREADS / 64) + wave) * (64 * CC_SIZE_STEPS);
  int carry_id = 0;  // wave-uniform
  unsigned long long carry_len = 0;
  for (int st = 0; st < CC_SIZE_STEPS; ++st) {
    const long long v = base + st * 64 + lane;
    if (base + st * 64 >= V) break;  // wave-uniform
    int id = 0;
    if (v < V) id = ids[v];
    PMU_DCHECK(id >= 0 && id <= n, PMU_DBG_INDEX);
    if (id < 0 || id > n) id = 0;
    const int prev = __shfl_up(id, 1, 64);
    const bool head = lane == 0 || id != prev;
    const unsigned long long heads = __ballot(head);
    const int id0 = __shfl(id, 0, 64);
    if (heads == 1ull && id0 == carry_id) {  // one run, the carried id (or more background)
      carry_len += 64;
      continue;
    }
    if (lane == 0 && carry_id) atomicAdd(size + (carry_id - 1), carry_len);
    carry_id = 0;
    carry_len = 0;
    if (heads == 1ull) {  // one run of a new id: carry it
      carry_id = id0;
      carry_len = 64;
      if (lane == 0 && id0) cls[id0 - 1] = lab[v];
      continue;
    }
    if (head && id) {
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
      atomicAdd(size + (id - 1), (unsigned long long)len);
      cls[id - 1] = lab[v];  // (every writer of a component stores the same value)
    }
  }
  if (lane == 0 && carry_id) atomicAdd(size + (carry_id - 1), carry_len);
}

__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const unsigned char* lab, const int* __restrict__ ids,
                                                               long long V, const unsigned char* __restrict__ keep,
                                                               long long n, unsigned char* out) {
  const long long stride = (long long)gridDim.x * CC_THREADS;
  for (long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x; v < V; v += stride) {
    const int id = ids[v];
    PMU_DCHECK(id >= 0 && id <= n, PMU_DBG_INDEX);
    unsigned char o = 0;
    if (id > 0 && id <= n && keep[id - 1]) o = lab[v];
    out[v] = o;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_overlap_kernel(const int* __restrict__ ids_a,
                                                                const unsigned char* __restrict__ lab_a,
                                                                long long n_a, const int* __restrict__ ids_b,
                                                                const unsigned char* __restrict__ lab_b,
                                                                long long n_b, long long V,
                                                                unsigned char* __restrict__ hit_a,
                                                                unsigned char* __restrict__ hit_b) {
  const long long stride = (long long)gridDim.x * CC_THREADS;
  for (long long v = (long long)blockIdx.x * CC_THREADS + threadIdx.x; v < V; v += stride) {
    const unsigned char a = lab_a[v];
    if (!a || a != lab_b[v]) continue;
    const int ia = ids_a[v], ib = ids_b[v];
    PMU_DCHECK(ia >= 0 && ia <= n_a && ib >= 0 && ib <= n_b, PMU_DBG_INDEX);
    if (ia > 0 && ia <= n_a) hit_a[ia - 1] = 1;
    if (ib > 0 && ib <= n_b) hit_b[ib - 1] = 1;
  }
}

size_t ws_for(long long V) {
  const long long nb = (V + CC_CHUNK - 1) / CC_CHUNK;
  return (size_t)((nb * 4 + 255) / 256 * 256);
}
bool dims_ok(int D0, int D1, int D2) {
  if (D0 < 1 || D0 > CC_MAXDIM || D1 < 1 || D1 > CC_MAXDIM || D2 < 1 || D2 > CC_MAXDIM) return false;
  return (long long)D0 * D1 * D2 < (1LL << 31);
}
bool count_ok(long long V, long long n) { return V >= 1 && V < (1LL << 31) && n >= 0 && n <= V; }

}  // namespace

extern "C" size_t pmu_cc_ws(int D0, int D1, int D2) {
  if (!dims_ok(D0, D1, D2)) return 0;
  return ws_for((long long)D0 * D1 * D2);
}

extern "C" int pmu_cc_label(const unsigned char* lab, int D0, int D1, int D2, int connectivity, int* root,
                            unsigned long long* n_components, void* ws, size_t ws_bytes, void* stream) {
  PMU_REQUIRE(lab && root && n_components && ws && dims_ok(D0, D1, D2));
  PMU_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26);
  PMU_REQUIRE(ws_bytes >= pmu_cc_ws(D0, D1, D2));
  const int maxnz = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  const long long V = (long long)D0 * D1 * D2;
  const int tiles0 = pmu_cdiv(D0, CC_T0), tiles1 = pmu_cdiv(D1, CC_T1), tiles2 = pmu_cdiv(D2, CC_T2);
  const long long tiles = (long long)tiles0 * tiles1 * tiles2;
  PMU_REQUIRE(tiles < (1LL << 31));
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(n_components, 0, sizeof(unsigned long long), st) != hipSuccess) return PMU_ERR_ARG;
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles), dim3(CC_THREADS), 0, st, lab, D0, D1, D2, maxnz, tiles1,
                     tiles2, root);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((V + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st,
                     lab, D0, D1, D2, maxnz, root);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_for(V)), dim3(CC_THREADS), 0, st, root, (int)V, n_components);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_cc_compact(const int* root, long long V, int* ids, unsigned long long* n, void* ws,
                              size_t ws_bytes, void* stream) {
  PMU_REQUIRE(root && ids && n && ws && V >= 1 && V < (1LL << 31));
  PMU_REQUIRE(ws_bytes >= ws_for(V));
  const long long nb = (V + CC_CHUNK - 1) / CC_CHUNK;
  unsigned* counts = static_cast<unsigned*>(ws);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)nb), dim3(CC_THREADS), 0, st, root, V, counts);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, counts, nb, n);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_mark_kernel, dim3((unsigned)nb), dim3(CC_THREADS), 0, st, root, V, counts, ids);
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_resolve_kernel, dim3(grid_for(V)), dim3(CC_THREADS), 0, st, ids, V);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_cc_sizes(const int* ids, const unsigned char* lab, long long V, long long n, long long* size,
                            unsigned char* cls, void* stream) {
  PMU_REQUIRE(ids && lab && count_ok(V, n) && ((size && cls) || n == 0));
  if (n == 0) return PMU_OK;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(size, 0, sizeof(long long) * (size_t)n, st) != hipSuccess) return PMU_ERR_ARG;
  if (hipMemsetAsync(cls, 0, (size_t)n, st) != hipSuccess) return PMU_ERR_ARG;
  const long long per_block = (long long)CC_THREADS * CC_SIZE_STEPS;
  hipLaunchKernelGGL(cc_sizes_kernel, dim3((unsigned)((V + per_block - 1) / per_block)), dim3(CC_THREADS), 0, st, ids,
                     lab, V, n, reinterpret_cast<unsigned long long*>(size), cls);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_cc_filter(const unsigned char* lab, const int* ids, long long V, const unsigned char* keep,
                             long long n, unsigned char* out, void* stream) {
  PMU_REQUIRE(lab && ids && out && count_ok(V, n) && (keep || n == 0));
  hipLaunchKernelGGL(cc_filter_kernel, dim3(grid_for(V)), dim3(CC_THREADS), 0, (hipStream_t)stream, lab, ids, V, keep,
                     n, out);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_cc_overlap(const int* ids_a, const unsigned char* lab_a, long long n_a, const int* ids_b,
                              const unsigned char* lab_b, long long n_b, long long V, unsigned char* hit_a,
                              unsigned char* hit_b, void* stream) {
  PMU_REQUIRE(ids_a && lab_a && ids_b && lab_b && count_ok(V, n_a) && count_ok(V, n_b));
  PMU_REQUIRE((hit_a || n_a == 0) && (hit_b || n_b == 0));
  hipStream_t st = (hipStream_t)stream;
  if (n_a && hipMemsetAsync(hit_a, 0, (size_t)n_a, st) != hipSuccess) return PMU_ERR_ARG;
  if (n_b && hipMemsetAsync(hit_b, 0, (size_t)n_b, st) != hipSuccess) return PMU_ERR_ARG;
  if (n_a == 0 || n_b == 0) return PMU_OK;  // nothing can touch
  hipLaunchKernelGGL(cc_overlap_kernel, dim3(grid_for(V)), dim3(CC_THREADS), 0, st, ids_a, lab_a, n_a, ids_b, lab_b,
                     n_b, V, hit_a, hit_b);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
