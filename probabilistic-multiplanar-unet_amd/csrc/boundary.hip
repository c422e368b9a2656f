// Boundary loss (Kervadec et al., MIDL 2019): the signed distance map of a batch of target planes
// (pmu_boundary_map) and the loss L = (1 / cnt) sum v p_k phi_k with its gradient (pmu_boundary_fwd / _bwd).
// The definition is in include/pmunet_hip.h; tests/boundary_ref.py restates it in numpy.
//
// Map.  Squared pixel distances are integers below 2^24, exact in fp32, so the minimum is exact whatever the
// order; the one rounding is the square root, and 1 - sqrt is a single fp32 subtraction (FP contraction off
// for the file): the map is a pure function of the target, bit-equal to the restatement.  The square root is
// sqrtf, which hipcc expands to v_sqrt_f32 plus the fma correction steps that round it correctly (its default
// -fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is, with this compiler's headers, the bare v_sqrt_f32
// (1 ulp), which the 300 x 300 test planes tell apart on one distance in six.
//   boundary_bits_kernel  reads the target once.  A wave turns 64 pixels of a row into one ballot word of
//           membership per class, bits[n][k][y][word] (one bit per pixel and class: 1/32 of the map's bytes),
//           and ORs a flag pair per plane (has a member, has a non-member: integer atomics).
//   boundary_map_kernel   a block owns one plane and a tile of TW columns by the whole height in LDS
//           (TW = 64 / 32 / 16 for H <= 256 / 512 / 1024: 64 KiB, two blocks per CU, as surface.hip's column
//           pass).  It rebuilds the row stage into the tile from the bit rows: the distance to the nearest
//           bit of the opposite membership by clz / ctz — the mask for a non-member, its complement limited
//           to the row width for a member — stored squared, with the pixel's membership as the sign (a row
//           distance is at least 1, so the sign is never lost).  One signed field serves both transforms: in
//           the column scan a pixel reads d^2 + 0 from a row whose pixel has the opposite sign and
//           d^2 + |stored| from one with its own.  The scan runs outward from the pixel and stops at the
//           first d^2 >= best: exact, d^2 is non-decreasing.  A thread scans four adjacent columns (one
//           ds_read_b128 per side and step).  phi is the only HBM write; a plane whose flag pair is not
//           (1, 1) is written as zeros.  No host synchronisation: the flags are read on the device.
//   The scan costs about 2 sqrt(d2) LDS reads per pixel: it, not the bytes, bounds the map (DESIGN.md
//   "Boundary loss").
//
// Loss.  As dice_loss.hip: grid (G, N), grid-stride pixels (four per 16-byte load where the planes are
// aligned), fp32 softmax, the products p phi and their sum in fp64 registers, the valid pixels as an integer
// count; a 64-lane butterfly per wave, the four waves through LDS in fixed order, one partial row per block;
// then one block sums the rows in a fixed order.  No float atomics: bit-identical runs.  Backward: one
// elementwise pass scaled by g / cnt read from the device.  HBM-bound: (8K + 8) N HW bytes forward,
// (12K + 8) N HW backward (K == 1: 8 and 12 N HW).
#include "pmu_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BD_MAXDIM = PMU_SURFACE_MAX_DIM;
constexpr int BD_MAXK = 8;
constexpr int BD_ROWS = 4;            // rows of one boundary_bits_kernel block
constexpr int BD_TILE = 16384;        // floats of a column tile: 64 KiB, two blocks per CU
constexpr int BD_CT = 512;            // threads of a boundary_map_kernel block
static_assert(2 * BD_TILE * 4 <= 160 * 1024, "two column tiles fit the LDS of a CU");
static_assert(BD_TILE / BD_MAXDIM >= 16, "the longest line fits a tile of at least 16 columns");

constexpr int BT = 256;               // threads of a loss block
constexpr int BFWD_BLOCKS = 1024;
constexpr int BBWD_BLOCKS = 2048;
constexpr int BFWD_PX = 2048;
constexpr int BBWD_PX = 1024;

typedef long long ll2 __attribute__((ext_vector_type(2)));

int grid_x(int N, long long HW, int px, int max_blocks) {
  long long g = (HW + px - 1) / px, cap = max_blocks / N;
  if (cap < 1) cap = 1;
  if (g > cap) g = cap;
  return (int)g;
}

bool shape_ok(int N, int K, int H, int W) {
  return N > 0 && N <= 65535 && K >= 1 && K <= BD_MAXK && H >= 1 && H <= BD_MAXDIM && W >= 1 && W <= BD_MAXDIM;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// workspace: [partials double N x G x 2 | flags u32 N x K (padded to 8 bytes) | bits u64 N x K x H x cw]
struct BdWs {
  double* part;
  unsigned* flags;
  unsigned long long* bits;
  size_t flags_bytes, bytes;
};
BdWs bd_ws(void* ws, int N, int K, int H, int W) {
  const int cw = (W + 63) >> 6;
  const size_t part_b = (size_t)N * grid_x(N, (long long)H * W, BFWD_PX, BFWD_BLOCKS) * 2 * sizeof(double);
  const size_t flags_b = (((size_t)N * K * sizeof(unsigned)) + 7) & ~(size_t)7;
  const size_t bits_b = (size_t)N * K * H * cw * sizeof(unsigned long long);
  char* b = (char*)ws;
  return BdWs{(double*)b, (unsigned*)(b + part_b), (unsigned long long*)(b + part_b + flags_b), flags_b,
              part_b + flags_b + bits_b};
}

// ------------------------------------------------------------------------------------------- map
// BIN: tgt float [N][H][W], member iff t >= 0.5 (K == 1).  Otherwise tgt int64 [N][H][W], member of class k
// iff t == k and t != ignore.
template <bool BIN>
__global__ __launch_bounds__(256) void boundary_bits_kernel(const void* __restrict__ tgt, int K, int H, int W,
                                                            long long ignore, unsigned long long* __restrict__ bits,
                                                            unsigned* __restrict__ flags) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y, cw = (W + 63) >> 6;
  const int y0 = blockIdx.x * BD_ROWS;
  PMU_DCHECK(y0 < H && cw <= BD_MAXDIM / 64 && K <= BD_MAXK, PMU_DBG_GRID);
  unsigned has_m = 0, has_o = 0;  // bit k: plane k has a member / a non-member among this wave's pixels
  for (int c = wave; c < BD_ROWS * cw; c += 4) {  // wave-uniform
    const int rr = c / cw, word = c - rr * cw;
    const int y = y0 + rr, j = word * 64 + lane;
    if (y >= H) break;
    const bool in = j < W;
    long long tv = -1;
    bool valid_t = false;
    if (in) {
      const long long p = ((long long)n * H + y) * W + j;
      PMU_DCHECK(p < (long long)gridDim.y * H * W, PMU_DBG_OPERAND);
      if constexpr (BIN) {
        tv = reinterpret_cast<const float*>(tgt)[p] >= 0.5f ? 0 : -1;
        valid_t = true;
      } else {
        tv = reinterpret_cast<const long long*>(tgt)[p];
        valid_t = tv != ignore;
      }
    }
    const unsigned long long row_bits = __ballot(in);
    for (int k = 0; k < K; ++k) {
      const unsigned long long m = __ballot(valid_t && tv == k);
      if (lane == 0) {
        const long long o = (((long long)n * K + k) * H + y) * cw + word;
        PMU_DCHECK(o < (long long)gridDim.y * K * H * cw, PMU_DBG_WORKSPACE);
        bits[o] = m;
      }
      has_m |= (m != 0ull ? 1u : 0u) << k;
      has_o |= ((row_bits & ~m) != 0ull ? 1u : 0u) << k;
    }
  }
  if (lane == 0)
    for (int k = 0; k < K; ++k) {
      const unsigned f = ((has_m >> k) & 1u) | (((has_o >> k) & 1u) << 1);
      if (f) atomicOr(&flags[n * K + k], f);
    }
}

__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(p);
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

// Block b owns plane b / tiles (= n K + k) and its columns x0 = (b % tiles) * TW .. x0 + TW, TW = 1 << tws,
// H * TW <= BD_TILE, TW % 4 == 0.  vec: W % 4 == 0 and phi 16-byte aligned (one 16-byte store per thread).
__global__ __launch_bounds__(BD_CT) void boundary_map_kernel(const unsigned long long* __restrict__ bits,
                                                             const unsigned* __restrict__ flags, int planes, int H,
                                                             int W, int tws, int tiles, int vec,
                                                             float* __restrict__ phi) {
  __shared__ __attribute__((aligned(16))) float tile[BD_TILE];
  const int tid = threadIdx.x, TW = 1 << tws;
  const int plane = (int)(blockIdx.x / (unsigned)tiles);
  const int x0 = (int)(blockIdx.x - (unsigned)plane * (unsigned)tiles) << tws;
  const int cw = (W + 63) >> 6;
  PMU_DCHECK(plane < planes && x0 < W && H * TW <= BD_TILE && TW >= 4, PMU_DBG_GRID);
  float* out = phi + (long long)plane * H * W;
  const int elems = H << tws;
  if (flags[plane] != 3u) {  // block-uniform: no member or no non-member, phi = 0 on the plane
    for (int e = tid; e < elems; e += BD_CT) {
      const int y = e >> tws, j = x0 + (e & (TW - 1));
      if (j < W) out[(long long)y * W + j] = 0.f;
    }
    return;
  }
  const unsigned long long* pb = bits + (long long)plane * H * cw;
  const unsigned long long tail = ~0ull >> ((64 - (W & 63)) & 63);  // the row's bits of its last word
  const float inf = __builtin_inff();
  // the row stage, from the bit rows into the tile: +r^2 for a member, -r^2 for a non-member, r the distance to
  // the nearest pixel of the row with the opposite membership (inf: none)
  for (int e = tid; e < elems; e += BD_CT) {
    const int y = e >> tws, j = x0 + (e & (TW - 1));
    float v = inf;  // columns past the plane: never scanned, never stored
    if (j < W) {
      const unsigned long long* row = pb + (long long)y * cw;
      const int word = j >> 6, bit = j & 63;
      PMU_DCHECK(((long long)plane * H + y) * cw + word < (long long)planes * H * cw, PMU_DBG_WORKSPACE);
      const unsigned long long own = row[word];
      const bool mem = (own >> bit) & 1ull;
      const unsigned long long flip = mem ? ~0ull : 0ull;  // the seeds of a member are the complement
      const unsigned long long upto = ~0ull >> (63 - bit);  // bits <= bit
      int dist = -1;
      unsigned long long m = (own ^ flip) & upto;
      for (int w = word;;) {
        if (m) {
          dist = j - (w * 64 + 63 - __builtin_clzll(m));
          break;
        }
        if (--w < 0) break;
        m = row[w] ^ flip;  // (a word left of another lies inside the row entirely)
      }
      m = (own ^ flip) & ~upto & (word == cw - 1 ? tail : ~0ull);
      for (int w = word;;) {
        if (m) {
          const int d = w * 64 + __builtin_ctzll(m) - j;
          if (dist < 0 || d < dist) dist = d;
          break;
        }
        if (++w >= cw) break;
        m = (row[w] ^ flip) & (w == cw - 1 ? tail : ~0ull);
      }
      PMU_DCHECK(dist != 0 && dist < W, PMU_DBG_INDEX);
      const float r2 = dist < 0 ? inf : (float)(dist * dist);
      v = mem ? r2 : -r2;
    }
    tile[e] = v;
  }
  __syncthreads();
  const int wvs = tws - 2;  // log2 of the 4-column groups of a tile row
  const int items = H << wvs;
  for (int i = tid; i < items; i += BD_CT) {
    const int y = i >> wvs, x = (i & ((1 << wvs) - 1)) << 2;
    if (x0 + x >= W) continue;
    const int e = (y << tws) + x;
    float b[4], s[4];
    bool neg[4], live[4];
    ld4(tile + e, s);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      b[c] = fabsf(s[c]);
      neg[c] = s[c] < 0.f;
      live[c] = x0 + x + c < W;
    }
    const int up = y, dn = H - 1 - y;
    const int far = up > dn ? up : dn;
    for (int d = 1; d <= far; ++d) {
      const float t = (float)(d * d);
      bool go = false;  // every candidate of this and any farther row is >= t
#pragma unroll
      for (int c = 0; c < 4; ++c) go = go || (live[c] && t < b[c]);
      if (!go) break;
      float q[4];
      if (d <= up) {
        PMU_DCHECK(e - (d << tws) >= 0, PMU_DBG_INDEX);
        ld4(tile + e - (d << tws), q);
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = fminf(b[c], __fadd_rn(t, (q[c] < 0.f) == neg[c] ? fabsf(q[c]) : 0.f));
      }
      if (d <= dn) {
        PMU_DCHECK(e + (d << tws) + 3 < elems, PMU_DBG_INDEX);
        ld4(tile + e + (d << tws), q);
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = fminf(b[c], __fadd_rn(t, (q[c] < 0.f) == neg[c] ? fabsf(q[c]) : 0.f));
      }
    }
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float dist = sqrtf(b[c]);  // correctly rounded (see the head of the file); not __fsqrt_rn
      r[c] = neg[c] ? dist : __fsub_rn(1.f, dist);
    }
    float* o = out + (long long)y * W + x0 + x;
    PMU_DCHECK((long long)plane * H * W + (long long)y * W + x0 + x < (long long)planes * H * W, PMU_DBG_OUTPUT);
    if (vec) {  // W % 4 == 0: the four columns are inside the plane
      *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (live[c]) o[c] = r[c];
    }
  }
}

// ------------------------------------------------------------------------------------------- loss
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// the sum over the wave in every lane, in the xor butterfly's order (dice_loss.hip).  Every lane active.
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// the block's (sum, valid count) into part[0..2): wave butterflies, then the four waves in order
__device__ __forceinline__ void block_sums(double s, unsigned cnt, double* __restrict__ part) {
  __shared__ double red[BT / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double a = wave_sum_f64(s), c = wave_sum_f64((double)cnt);
  if (lane == 0) {
    red[wave][0] = a;
    red[wave][1] = c;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    part[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

template <int K>
__device__ __forceinline__ void softmax_px(const float (&xv)[K], float (&p)[K]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) m = fmaxf(m, xv[k]);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    p[k] = expf(xv[k] - m);
    se += p[k];
  }
  const float inv = 1.f / se;
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] *= inv;
}

template <int K>
__device__ __forceinline__ void mc_fwd_px(const float (&xv)[K], const float (&fv)[K], long long tv, long long ignore,
                                          int first, double& s, unsigned& cnt) {
  if (tv == ignore) return;
  float p[K];
  softmax_px<K>(xv, p);
  ++cnt;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (k >= first) s += (double)p[k] * (double)fv[k];
}

// x, phi [N][K][HW], tgt [N][HW]; part[n][blockIdx.x][2]
template <int K>
__global__ __launch_bounds__(BT) void boundary_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                          const float* __restrict__ phi, long long HW, long long ignore,
                                                          int first, int vec, double* __restrict__ part) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * K * HW;
  const float* fn = phi + (long long)n * K * HW;
  const long long* tn = tgt + (long long)n * HW;
  double s = 0.0;
  unsigned cnt = 0u;
  const long long t0 = (long long)blockIdx.x * BT + threadIdx.x, step = (long long)gridDim.x * BT;
  float xv[K], fv[K];
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      float4 v[K], f[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        v[k] = pmu_ld4(xn + k * HW + 4 * q);
        f[k] = pmu_ld4(fn + k * HW + 4 * q);
      }
      const ll2 ta = *reinterpret_cast<const ll2*>(tn + 4 * q), tb = *reinterpret_cast<const ll2*>(tn + 4 * q + 2);
#pragma unroll
      for (int k = 0; k < K; ++k) { xv[k] = v[k].x; fv[k] = f[k].x; }
      mc_fwd_px<K>(xv, fv, ta.x, ignore, first, s, cnt);
#pragma unroll
      for (int k = 0; k < K; ++k) { xv[k] = v[k].y; fv[k] = f[k].y; }
      mc_fwd_px<K>(xv, fv, ta.y, ignore, first, s, cnt);
#pragma unroll
      for (int k = 0; k < K; ++k) { xv[k] = v[k].z; fv[k] = f[k].z; }
      mc_fwd_px<K>(xv, fv, tb.x, ignore, first, s, cnt);
#pragma unroll
      for (int k = 0; k < K; ++k) { xv[k] = v[k].w; fv[k] = f[k].w; }
      mc_fwd_px<K>(xv, fv, tb.y, ignore, first, s, cnt);
    }
  } else {
    for (long long p = t0; p < HW; p += step) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        xv[k] = xn[k * HW + p];
        fv[k] = fn[k * HW + p];
      }
      mc_fwd_px<K>(xv, fv, tn[p], ignore, first, s, cnt);
    }
  }
  block_sums(s, cnt, part + ((long long)n * gridDim.x + blockIdx.x) * 2);
}

__device__ __forceinline__ float bin_prob(float xv, int act) { return act ? 1.f / (1.f + expf(-xv)) : xv; }

// K == 1: x [N][HW] a probability (act 0) or a logit (act 1), phi [N][HW]; every pixel is valid
__global__ __launch_bounds__(BT) void boundary_fwd_bin_kernel(const float* __restrict__ x, const float* __restrict__ phi,
                                                              long long HW, int act, int vec,
                                                              double* __restrict__ part) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * HW;
  const float* fn = phi + (long long)n * HW;
  double s = 0.0;
  unsigned cnt = 0u;
  const long long t0 = (long long)blockIdx.x * BT + threadIdx.x, step = (long long)gridDim.x * BT;
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      const float4 xv = pmu_ld4(xn + 4 * q), fv = pmu_ld4(fn + 4 * q);
      s += (double)bin_prob(xv.x, act) * (double)fv.x;
      s += (double)bin_prob(xv.y, act) * (double)fv.y;
      s += (double)bin_prob(xv.z, act) * (double)fv.z;
      s += (double)bin_prob(xv.w, act) * (double)fv.w;
      cnt += 4u;
    }
  } else {
    for (long long p = t0; p < HW; p += step) {
      s += (double)bin_prob(xn[p], act) * (double)fn[p];
      ++cnt;
    }
  }
  block_sums(s, cnt, part + ((long long)n * gridDim.x + blockIdx.x) * 2);
}

// One block: the rows of part[rows][2] added up in a fixed order (thread t rows t, t + BT, ... in order, then a
// tree over the threads); cnt = valid pixels x classes, loss = S / cnt (0 when cnt == 0).
__global__ __launch_bounds__(BT) void boundary_final_kernel(const double* __restrict__ part, int rows, int classes,
                                                            float* __restrict__ loss, double* __restrict__ count) {
  __shared__ double ra[BT], rb[BT];
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int r = tid; r < rows; r += BT) {
    a += part[2 * (long long)r];
    b += part[2 * (long long)r + 1];
  }
  ra[tid] = a;
  rb[tid] = b;
  __syncthreads();
  for (int o = BT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      ra[tid] += ra[tid + o];
      rb[tid] += rb[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double cnt = rb[0] * (double)classes;
    count[0] = cnt;
    loss[0] = cnt > 0.0 ? (float)(ra[0] / cnt) : 0.f;
  }
}

// g / cnt in fp32 (0 when nothing is valid)
__device__ __forceinline__ float grad_scale(const float* __restrict__ gout, const double* __restrict__ count) {
  const double cnt = count[0];
  return cnt > 0.0 ? (float)((double)gout[0] / cnt) : 0.f;
}

template <int K>
__device__ __forceinline__ void mc_bwd_px(const float (&xv)[K], const float (&fv)[K], long long tv, long long ignore,
                                          int first, float gs, float (&out)[K]) {
  if (tv == ignore) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = 0.f;
    return;
  }
  float p[K], c[K], dot = 0.f;
  softmax_px<K>(xv, p);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    c[k] = k >= first ? fv[k] : 0.f;
    dot = fmaf(p[k], c[k], dot);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = gs * p[k] * (c[k] - dot);
}

template <int K>
__global__ __launch_bounds__(BT) void boundary_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                          const float* __restrict__ phi, long long HW, long long ignore,
                                                          int first, const float* __restrict__ gout,
                                                          const double* __restrict__ count, int vec,
                                                          float* __restrict__ dx) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * K * HW;
  const float* fn = phi + (long long)n * K * HW;
  float* dn = dx + (long long)n * K * HW;
  const long long* tn = tgt + (long long)n * HW;
  const float gs = grad_scale(gout, count);
  const long long t0 = (long long)blockIdx.x * BT + threadIdx.x, step = (long long)gridDim.x * BT;
  float xv[K], fv[K], o[K];
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      float4 v[K], f[K], r[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        v[k] = pmu_ld4(xn + k * HW + 4 * q);
        f[k] = pmu_ld4(fn + k * HW + 4 * q);
      }
      const ll2 ta = *reinterpret_cast<const ll2*>(tn + 4 * q), tb = *reinterpret_cast<const ll2*>(tn + 4 * q + 2);
#pragma unroll
      for (int k = 0; k < K; ++k) { xv[k] = v[k].x; fv[k] = f[k].x; }
      mc_bwd_px<K>(xv, fv, ta.x, ignore, first, gs, o);
#pragma unroll
      for (int k = 0; k < K; ++k) { r[k].x = o[k]; xv[k] = v[k].y; fv[k] = f[k].y; }
      mc_bwd_px<K>(xv, fv, ta.y, ignore, first, gs, o);
#pragma unroll
      for (int k = 0; k < K; ++k) { r[k].y = o[k]; xv[k] = v[k].z; fv[k] = f[k].z; }
      mc_bwd_px<K>(xv, fv, tb.x, ignore, first, gs, o);
#pragma unroll
      for (int k = 0; k < K; ++k) { r[k].z = o[k]; xv[k] = v[k].w; fv[k] = f[k].w; }
      mc_bwd_px<K>(xv, fv, tb.y, ignore, first, gs, o);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        r[k].w = o[k];
        *reinterpret_cast<float4*>(dn + k * HW + 4 * q) = r[k];
      }
    }
  } else {
    for (long long p = t0; p < HW; p += step) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        xv[k] = xn[k * HW + p];
        fv[k] = fn[k * HW + p];
      }
      mc_bwd_px<K>(xv, fv, tn[p], ignore, first, gs, o);
#pragma unroll
      for (int k = 0; k < K; ++k) dn[k * HW + p] = o[k];
    }
  }
}

// dx = gs phi (act 0) or gs phi p (1 - p) (act 1)
__device__ __forceinline__ float bin_bwd_px(float xv, float fv, int act, float gs) {
  const float c = gs * fv;
  if (!act) return c;
  const float p = bin_prob(xv, 1);
  return c * p * (1.f - p);
}

__global__ __launch_bounds__(BT) void boundary_bwd_bin_kernel(const float* __restrict__ x, const float* __restrict__ phi,
                                                              long long HW, int act, const float* __restrict__ gout,
                                                              const double* __restrict__ count, int vec,
                                                              float* __restrict__ dx) {
  const int n = blockIdx.y;
  const float* xn = x + (long long)n * HW;
  const float* fn = phi + (long long)n * HW;
  float* dn = dx + (long long)n * HW;
  const float gs = grad_scale(gout, count);
  const long long t0 = (long long)blockIdx.x * BT + threadIdx.x, step = (long long)gridDim.x * BT;
  if (vec) {
    const long long Q = HW >> 2;
    for (long long q = t0; q < Q; q += step) {
      const float4 xv = pmu_ld4(xn + 4 * q), fv = pmu_ld4(fn + 4 * q);
      float4 r;
      r.x = bin_bwd_px(xv.x, fv.x, act, gs);
      r.y = bin_bwd_px(xv.y, fv.y, act, gs);
      r.z = bin_bwd_px(xv.z, fv.z, act, gs);
      r.w = bin_bwd_px(xv.w, fv.w, act, gs);
      *reinterpret_cast<float4*>(dn + 4 * q) = r;
    }
  } else {
    for (long long p = t0; p < HW; p += step) dn[p] = bin_bwd_px(xn[p], fn[p], act, gs);
  }
}

bool loss_shape_ok(int N, int K, long long HW) {
  return N > 0 && N <= 65535 && K >= 1 && K <= BD_MAXK && HW > 0 && HW <= (long long)BD_MAXDIM * BD_MAXDIM;
}

}  // namespace

#define BD_FOR_K(K, CALL)   \
  switch (K) {              \
    case 2: CALL(2); break; \
    case 3: CALL(3); break; \
    case 4: CALL(4); break; \
    case 5: CALL(5); break; \
    case 6: CALL(6); break; \
    case 7: CALL(7); break; \
    default: CALL(8); break; \
  }

extern "C" size_t pmu_boundary_ws(int N, int K, int H, int W) {
  if (!shape_ok(N, K, H, W)) return 0;
  return bd_ws(nullptr, N, K, H, W).bytes;
}

extern "C" int pmu_boundary_map(const void* tgt, int kind, int N, int K, int H, int W, long long ignore_index,
                                float* phi, void* ws, void* stream) {
  PMU_REQUIRE(tgt && phi && ws && shape_ok(N, K, H, W));
  PMU_REQUIRE((kind == 0 && K >= 2) || (kind == 1 && K == 1));
  PMU_REQUIRE(((uintptr_t)ws & 7) == 0);
  const BdWs w = bd_ws(ws, N, K, H, W);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(w.flags, 0, w.flags_bytes, st) != hipSuccess) return PMU_ERR_ARG;
  const dim3 bgrid((unsigned)((H + BD_ROWS - 1) / BD_ROWS), (unsigned)N);
  if (kind == 1)
    hipLaunchKernelGGL(boundary_bits_kernel<true>, bgrid, dim3(256), 0, st, tgt, K, H, W, ignore_index, w.bits, w.flags);
  else
    hipLaunchKernelGGL(boundary_bits_kernel<false>, bgrid, dim3(256), 0, st, tgt, K, H, W, ignore_index, w.bits,
                       w.flags);
  PMU_CHECK_LAUNCH();
  const int tws = H <= BD_TILE / 64 ? 6 : H <= BD_TILE / 32 ? 5 : 4;  // 64, 32 or 16 columns by the whole height
  const int tiles = (W + (1 << tws) - 1) >> tws;
  const long long blocks = (long long)N * K * tiles;
  PMU_REQUIRE(blocks >= 1 && blocks < (1LL << 31));
  const int vec = W % 4 == 0 && aligned16(phi);
  hipLaunchKernelGGL(boundary_map_kernel, dim3((unsigned)blocks), dim3(BD_CT), 0, st,
                     (const unsigned long long*)w.bits, (const unsigned*)w.flags, N * K, H, W, tws, tiles, vec, phi);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_boundary_fwd(const float* x, const void* tgt, const float* phi, int N, int K, long long HW, int act,
                                int first_class, long long ignore_index, float* loss, double* count, void* ws,
                                void* stream) {
  PMU_REQUIRE(x && phi && loss && count && ws && loss_shape_ok(N, K, HW) && (tgt || K == 1));
  PMU_REQUIRE((act == 0 || act == 1) && (first_class == 0 || first_class == 1));
  PMU_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)count & 7) == 0);
  double* part = (double*)ws;  // the head of the pmu_boundary_ws layout
  const int G = grid_x(N, HW, BFWD_PX, BFWD_BLOCKS);
  const int vec = HW % 4 == 0 && aligned16(x) && aligned16(phi) && (K == 1 || aligned16(tgt));
  const int first = K == 1 ? 0 : first_class;
  hipStream_t st = (hipStream_t)stream;
  if (K == 1) {
    hipLaunchKernelGGL(boundary_fwd_bin_kernel, dim3(G, N), dim3(BT), 0, st, x, phi, HW, act, vec, part);
  } else {
#define BD_FWD(KK)                                                                                                 \
  hipLaunchKernelGGL(boundary_fwd_kernel<KK>, dim3(G, N), dim3(BT), 0, st, x, (const long long*)tgt, phi, HW,       \
                     ignore_index, first, vec, part)
    BD_FOR_K(K, BD_FWD)
#undef BD_FWD
  }
  PMU_CHECK_LAUNCH();
  hipLaunchKernelGGL(boundary_final_kernel, dim3(1), dim3(BT), 0, st, (const double*)part, N * G, K - first, loss,
                     count);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}

extern "C" int pmu_boundary_bwd(const float* x, const void* tgt, const float* phi, int N, int K, long long HW, int act,
                                int first_class, long long ignore_index, const float* gout, const double* count,
                                float* dx, void* stream) {
  PMU_REQUIRE(x && phi && gout && count && dx && loss_shape_ok(N, K, HW) && (tgt || K == 1));
  PMU_REQUIRE((act == 0 || act == 1) && (first_class == 0 || first_class == 1));
  PMU_REQUIRE(((uintptr_t)count & 7) == 0);
  const int G = grid_x(N, HW, BBWD_PX, BBWD_BLOCKS);
  const int vec = HW % 4 == 0 && aligned16(x) && aligned16(phi) && aligned16(dx) && (K == 1 || aligned16(tgt));
  hipStream_t st = (hipStream_t)stream;
  if (K == 1) {
    hipLaunchKernelGGL(boundary_bwd_bin_kernel, dim3(G, N), dim3(BT), 0, st, x, phi, HW, act, gout, count, vec, dx);
  } else {
#define BD_BWD(KK)                                                                                                 \
  hipLaunchKernelGGL(boundary_bwd_kernel<KK>, dim3(G, N), dim3(BT), 0, st, x, (const long long*)tgt, phi, HW,       \
                     ignore_index, first_class, gout, count, vec, dx)
    BD_FOR_K(K, BD_BWD)
#undef BD_BWD
  }
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
