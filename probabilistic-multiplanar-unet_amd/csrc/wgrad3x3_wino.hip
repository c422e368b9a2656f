// Weight gradient of the 3x3 / pad 1 convolution in fp32 by Winograd F(2x2, 3x3) (the autograd of
// nn.Conv2d w.r.t. its weight, PMU/model/unet/unet_parts.py:15,18), on the materialised operands the
// forward and input-gradient kernels tee (xt = the conv's input operand, dzt = dL/dz; both NHWC fp32).
//
// For a 2x2 output tile with gradient block dY (per output channel) and 4x4 input patch X (per input
// channel), the forward is Y = A^T [(G g G^T) .* (B^T X B)] A, so
//     dL/dg = G^T [ (A dY A^T) .* (B^T X B) ] G     (summed over tiles)
// i.e. 16 per-component GEMMs over the tiles, M[c][co][ci] = sum_t Z[c][t][co] V[c][t][ci] with
// Z = A dY A^T, V = B^T X B, followed by the 3x4x4x3 output transform G^T M G — 16 products per tile
// and channel pair where the direct sum takes 36.  fp32 throughout; the result differs from the
// direct sum by fp32 rounding only.
//
// Block: 1024 threads, 64 output x 64 input channels (512 threads, 32 output channels where Cout is no
// multiple of 64), all 16 components, split by component row over the waves (wgrad3x3_wino32_kernel
// below).  K = tiles, in K-tiles of 128 output pixels (8 x 16 = 32 Winograd tiles, 8 MFMA steps);
// the next K-tile's dzt / xt images are fetched by LDS-DMA during the current one's MFMAs
// (double-buffered LDS, 145 KB): buffer loads through SGPR descriptors with scalar row addresses
// (wgw_sdma), or global_load_lds with per-lane addresses for operands of 2^31 bytes or more (wgw_dma).
// Split-K over blocks: each writes M for its tile range to a slab, and the
// reduce kernel sums the slabs in a fixed order (deterministic) and applies G^T M G.
#include <stdlib.h>
#include <string.h>
#include "pmu_common.h"
#include "pmu_lds.h"

namespace {

constexpr int NT = 512;
constexpr int WCO = 32, WCI = 64;        // channels per block
constexpr int TH = 8, TW = 16;           // output pixels per K-tile
constexpr int HH = TH + 2, HWD = TW + 2; // 10 x 18 operand halo
// LDS floats per dz / x pixel: unpadded — the kernel's 32-lane read groups all read one pixel's
// consecutive channels (conflict-free at any pitch), and the DMA then moves no pad units.
constexpr int XLS = WCI;
constexpr int X_FLOATS = HH * HWD * XLS;

struct WgwArgs {
  const float* dz;  // [N][H][W][Cout]
  const float* x;   // [N][H][W][Cin]
  float* ws;        // [nsplit][16][Cout][Cin]
  int N, H, W, Cout, Cin, tiles_w, tiles_h, ntiles, nsplit, nco;
};

__device__ __forceinline__ void wgw_origin(const WgwArgs& a, int tile, int& n, int& h0, int& w0) {
  int t = tile;
  const int tw = t % a.tiles_w; t /= a.tiles_w;
  const int th = t % a.tiles_h; t /= a.tiles_h;
  n = t; h0 = th * TH; w0 = tw * TW;
  PMU_DCHECK(n < a.N, PMU_DBG_GRID);
}

// LDS-DMA staging of one K-tile with per-lane addresses (operands of 2^31 bytes or more, else wgw_sdma
// below): the slot is the dz image (128 px x 8 units) followed by the
// x halo image (180 px x 16 units); each global_load_lds wave-instruction fills 64 consecutive
// units, its lanes' global sources chosen per unit.  Units outside the input are zeroed with a
// ds_write instead (their DMA lanes masked); pad units are not written.
constexpr int X_UPX = XLS / 4;

// block geometry by output-channel width: 32 (512 threads) or 64 (1024 threads: 4 waves per SIMD,
// the x halo image shared by twice the output channels)
template <int WCO_>
struct WgwCfg {
  static constexpr int WCO = WCO_, NT = 16 * WCO_, DLS = WCO_;
  static constexpr int D_FLOATS = TH * TW * DLS;
  static constexpr int SLOT = D_FLOATS + X_FLOATS;
  static constexpr int D_UPX = DLS / 4;
  static constexpr int D_UNITS = TH * TW * D_UPX;
  static constexpr int W_UNITS = D_UNITS + HH * HWD * X_UPX;
  static constexpr int W_NGL = (W_UNITS + NT - 1) / NT;
  static_assert(D_UNITS * 4 == D_FLOATS && W_UNITS * 4 == SLOT, "slot = dz image + x image");
};

template <int WCO_>
__device__ __forceinline__ void wgw_dma(const WgwArgs& a, int tile, int co0, int ci0, int tid, float* slot) {
  using C = WgwCfg<WCO_>;
  int n, h0, w0;
  wgw_origin(a, tile, n, h0, w0);
  const int wbase = (tid >> 6) * 256;
#pragma unroll
  for (int r = 0; r < C::W_NGL; ++r) {
    const int u = r * C::NT + tid;
    // dz image unit (u < D_UNITS) or x halo unit, branch-free
    const bool isd = u < C::D_UNITS;
    const int pd = u / C::D_UPX, qd = u - pd * C::D_UPX;
    const int v = u - C::D_UNITS;
    const int px = v / X_UPX, qx = v - px * X_UPX;
    const int hr = px / HWD, hc = px - hr * HWD;
    const int h = isd ? h0 + (pd >> 4) : h0 - 1 + hr;
    const int w = isd ? w0 + (pd & 15) : w0 - 1 + hc;
    const bool data = isd ? qd < C::WCO / 4 : (u < C::W_UNITS && qx < WCI / 4);
    const bool in = data && h >= 0 && w >= 0 && h < a.H && w < a.W;
    const long long pix = ((long long)n * a.H + h) * a.W + w;
    PMU_DCHECK(!in || pix < (long long)a.N * a.H * a.W, PMU_DBG_OPERAND);
    const float* src = isd ? a.dz + pix * a.Cout + co0 + 4 * qd : a.x + pix * a.Cin + ci0 + 4 * qx;
    if (in)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(slot + 4 * r * C::NT + wbase), 16, 0, 0);
    else if (data)
      *reinterpret_cast<float4*>(slot + 4 * u) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ---------------------------------------------------------------------------------------------
// The kernel, on v_mfma_f32_32x32x2_f32: wave w owns component row i = w & 3
// (components 4i..4i+3) for 32 output x 32 input channels (half w >> 2 of the block's 64), acc[4] of
// 32x32 (64 registers).  A step covers 2 Winograd tiles (k = lane >> 5).  Row i of B^T X B needs
// only 2 of the 4 patch rows (tt = x[ra] +- x[rb]) and row i of A dY A^T one combination of the
// dz rows, so a step costs 10-12 LDS reads and 11-13 VALU for 4 MFMAs of 64 cycles.  The K loop is a template on the row (a wave-uniform
// switch picks it): the row's coefficients are then signs in the instructions, not multiplies.
// ---------------------------------------------------------------------------------------------
constexpr int NSTEP2 = (TH / 2) * (TW / 2) / 2;  // 2 tiles per step

struct WgwOps2 {
  float d[4];   // dz 2x2 of (tile, co) (row 0 reads d[0..1] only, row 3 d[2..3] only)
  float xa[4];  // patch row ra of (tile, ci)
  float xb[4];  // patch row rb
};

// K-tile staging by scalar-addressed LDS-DMA (buffer_load_dwordx4 ... lds through SGPR descriptors, as
// wgrad3x3_bf16_dma.hip).  The slot layout is wgw_dma's: the dz image, then the x halo image, unpadded.
// It is cut into wave-instructions of 64 units that each lie in ONE image row: a dz tile row is D_IPR whole
// instructions; an 18-pixel halo row is four whole ones and a fifth whose upper 32 lanes are switched off
// (the next row starts right behind its two pixels).  Instruction j of a K-tile belongs to wave j % NW.
// Its byte address = descriptor base (the tensor) + soffset (SGPR: image row and first pixel of the
// instruction) + voffset (VGPR: the lane's pixel and channel within the instruction, set once per kernel);
// its num_records are the tensor's bytes up to the end of that image row, so lanes past the right edge read
// zeros through the range check (gfx9 raw buffers: soffset + voffset >= num_records), and 0 for a row above
// or below the image.  The column left of the image (halo pixel 0 of tile column 0) cannot be reached that
// way: there the instruction starts at pixel 0 and takes the second per-lane offset vxl, one pixel less,
// with 0x80000000 in the lanes of halo pixel 0 (operands < 2^31 bytes, pmu_conv3x3_wgrad_wino_dma_ok: the
// sum with soffset neither wraps nor stays below any num_records).  A K-tile's issue is SALU work and the DMA
// instructions; nothing is written by ds_write.  (Descriptor inputs and soffset go through readfirstlane:
// see wgrad3x3_bf16_dma.hip on what the compiler does with values it cannot prove uniform.)
template <int WCO_>
struct WgwSd {
  using C = WgwCfg<WCO_>;
  static constexpr int NW = C::NT / 64;
  static constexpr int D_PPI = 64 / C::D_UPX;                // pixels per dz instruction (8 / 4)
  static constexpr int D_IPR = TW / D_PPI;                   // dz instructions per tile row (2 / 4)
  static constexpr int D_NI = TH * D_IPR;
  static constexpr int X_PPI = 64 / X_UPX;                   // pixels per x instruction (4)
  static constexpr int X_IPR = (HWD + X_PPI - 1) / X_PPI;    // x instructions per halo row (5)
  static constexpr int X_TAIL = (HWD - (X_IPR - 1) * X_PPI) * X_UPX;  // lanes of a halo row's last one (32)
  static constexpr int X_NI = HH * X_IPR;
  static constexpr int NI = D_NI + X_NI;
  static constexpr int NR = (NI + NW - 1) / NW;              // rounds per wave
  static_assert(64 % C::D_UPX == 0 && TW % D_PPI == 0 && 64 % X_UPX == 0, "instructions of whole pixels");
  static_assert(D_NI % NW == 0, "a round is all dz or all x");
};

struct WgwLane {
  unsigned vd, vx, vxl;  // voffset: dz; x; x of an instruction that starts at image column 0 for halo pixel 0
};

template <int WCO_>
__device__ __forceinline__ void wgw_sdma(const WgwArgs& a, int n, int th, int tw, int wave, int lane,
                                         const WgwLane& v, float* slot) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the descriptor type and builtins exist for the device pass only)
  using C = WgwCfg<WCO_>;
  using S = WgwSd<WCO_>;
  const int h0 = th * TH, w0 = tw * TW;
  const int row0 = n * a.H;
#pragma unroll
  for (int r = 0; r < S::NR; ++r) {
    const int j = r * S::NW + wave;  // (uniform)
    if (r * S::NW < S::D_NI) {
      const int dr = j / S::D_IPR;
      const int h = h0 + dr, w = w0 + (j - dr * S::D_IPR) * S::D_PPI;   // (never negative)
      const bool ok = h < a.H && w < a.W;
      const unsigned off = ((unsigned)(row0 + h) * (unsigned)a.W + (unsigned)w) * (unsigned)a.Cout * 4u;
      const int soff = __builtin_amdgcn_readfirstlane(ok ? (int)off : 0);
      const int nrec = __builtin_amdgcn_readfirstlane(ok ? (row0 + h + 1) * a.W * a.Cout * 4 : 0);
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dz), 0, nrec, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(slot + j * 256), 16, v.vd,
                                               soff, 0, 0);
    } else if (j < S::NI) {
      const int jx = j - S::D_NI;
      const int hr = jx / S::X_IPR, k = jx - hr * S::X_IPR;
      const int h = h0 - 1 + hr;
      const int wl = w0 - 1 + k * S::X_PPI;
      const bool left = wl < 0;       // (uniform: k == 0 of tile column 0)
      const int w = left ? 0 : wl;
      const bool ok = (unsigned)h < (unsigned)a.H && w < a.W;
      const unsigned off = ((unsigned)(row0 + h) * (unsigned)a.W + (unsigned)w) * (unsigned)a.Cin * 4u;
      const int soff = __builtin_amdgcn_readfirstlane(ok ? (int)off : 0);
      const int nrec = __builtin_amdgcn_readfirstlane(ok ? (row0 + h + 1) * a.W * a.Cin * 4 : 0);
      const unsigned vo = left ? v.vxl : v.vx;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, nrec, 0x00020000);
      float* dst = slot + C::D_FLOATS + (hr * HWD * X_UPX + k * 64) * 4;
      // (the fifth instruction of a halo row: two pixels; the lanes behind them would land in the next row)
      if (lane < (k == S::X_IPR - 1 ? S::X_TAIL : 64))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)dst, 16, vo, soff, 0, 0);
    }
  }
#else
  (void)a; (void)n; (void)th; (void)tw; (void)wave; (void)lane; (void)v; (void)slot;
#endif
}

// Row ROW of B^T = x[RA] + SX x[RB] and of A dY: rows 0 / 3 take dY row 0 / minus row 1, rows 1 / 2 their
// sum / difference.  Operand reads are explicit ds_read_b32 (asm): the compiler's own waits put an
// lgkmcnt(0) right after each step's read-ahead (its counter bookkeeping gave up), exposing the LDS latency
// every step.  Here a step waits for its operands — read one step earlier — before issuing the next step's
// reads, as the forward kernel does.  Per lane two base addresses per K-tile (the dz image and the lower of
// the two patch rows); step, value and patch row are immediate offsets of the ds_read (all below 64 KB).
// Step s covers tiles t = 2s + h (h = lane >> 5): ty = s >> 2, tx = 2 (s & 3) + h.
template <int ROW>
struct WgwRow {
  static constexpr int RA = ROW == 0 ? 0 : ROW == 2 ? 2 : 1;
  static constexpr int RB = ROW == 0 ? 2 : ROW == 1 ? 2 : ROW == 2 ? 1 : 3;
  static constexpr int RLO = RA < RB ? RA : RB;
  static constexpr int XA_OFF = 4 * (RA - RLO) * HWD * XLS, XB_OFF = 4 * (RB - RLO) * HWD * XLS;  // bytes
};

template <int WCO_, int ROW, int S>
__device__ __forceinline__ void wgw_read2(unsigned dbase, unsigned xbase, WgwOps2& o) {
  using C = WgwCfg<WCO_>;
  using R = WgwRow<ROW>;
  constexpr int DSTEP = 4 * ((2 * (S >> 2) * TW + 4 * (S & 3)) * C::DLS);
  constexpr int XSTEP = 4 * ((2 * (S >> 2) * HWD + 4 * (S & 3)) * XLS);
  static_assert(DSTEP + 4 * (TW + 1) * C::DLS < 65536 && XSTEP + 4 * 2 * HWD * XLS + 12 * XLS < 65536, "ds_read offset field");
  if constexpr (ROW != 3) {
    o.d[0] = lds_b32<DSTEP>(dbase);
    o.d[1] = lds_b32<DSTEP + 4 * C::DLS>(dbase);
  }
  if constexpr (ROW != 0) {
    o.d[2] = lds_b32<DSTEP + 4 * TW * C::DLS>(dbase);
    o.d[3] = lds_b32<DSTEP + 4 * (TW + 1) * C::DLS>(dbase);
  }
  o.xa[0] = lds_b32<XSTEP + R::XA_OFF>(xbase);
  o.xa[1] = lds_b32<XSTEP + R::XA_OFF + 4 * XLS>(xbase);
  o.xa[2] = lds_b32<XSTEP + R::XA_OFF + 8 * XLS>(xbase);
  o.xa[3] = lds_b32<XSTEP + R::XA_OFF + 12 * XLS>(xbase);
  o.xb[0] = lds_b32<XSTEP + R::XB_OFF>(xbase);
  o.xb[1] = lds_b32<XSTEP + R::XB_OFF + 4 * XLS>(xbase);
  o.xb[2] = lds_b32<XSTEP + R::XB_OFF + 8 * XLS>(xbase);
  o.xb[3] = lds_b32<XSTEP + R::XB_OFF + 12 * XLS>(xbase);
}

// steps S .. NSTEP2-1 of a K-tile (compile-time recursion: the step is part of the read offsets)
template <int WCO_, int ROW, int S>
__device__ __forceinline__ void wgw_steps2(unsigned dbase, unsigned xbase, WgwOps2 (&ops)[2], f32x16 (&acc)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // step S's operands (read one step ago)
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (S + 1 < NSTEP2) wgw_read2<WCO_, ROW, S + 1>(dbase, xbase, ops[(S + 1) & 1]);
  __builtin_amdgcn_sched_barrier(0);
  const WgwOps2& o = ops[S & 1];
  // Z row: r = the row's combination of dY rows 0, 1 (2 columns), then [r0, r0 + r1, r0 - r1, -r1]
  float r0, r1;
  if constexpr (ROW == 0) { r0 = o.d[0]; r1 = o.d[1]; }
  else if constexpr (ROW == 1) { r0 = o.d[0] + o.d[2]; r1 = o.d[1] + o.d[3]; }
  else if constexpr (ROW == 2) { r0 = o.d[0] - o.d[2]; r1 = o.d[1] - o.d[3]; }
  else { r0 = -o.d[2]; r1 = -o.d[3]; }
  float z[4] = {r0, r0 + r1, r0 - r1, -r1};
  // V row: tt = x[ra] +- x[rb], then [t0 - t2, t1 + t2, t2 - t1, t1 - t3]
  float tt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tt[j] = ROW == 1 ? o.xa[j] + o.xb[j] : o.xa[j] - o.xb[j];
  float v[4] = {tt[0] - tt[2], tt[1] + tt[2], tt[2] - tt[1], tt[1] - tt[3]};
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = mfma_f32_32x32x2(z[k], v[k], acc[k]);
  __builtin_amdgcn_sched_barrier(0);  // the next step's wait stays behind these MFMAs
  if constexpr (S + 1 < NSTEP2) wgw_steps2<WCO_, ROW, S + 1>(dbase, xbase, ops, acc);
}

// The K loop of one wave: K-tiles t_beg .. t_end-1 in order, the next one's staging issued before the
// current one's MFMA steps.  SDMA: scalar-addressed staging with a tile cursor (tile column, tile row,
// image) advanced per K-tile; else wgw_dma's per-lane addresses (operands of 2^31 bytes or more).
template <int WCO_, bool SDMA, int ROW>
__device__ __forceinline__ void wgw_kloop(const WgwArgs& a, float* smem, int t_beg, int t_end, int co0, int ci0, int tid,
                                          int wave, int half, int cg, f32x16 (&acc)[4]) {
  using C = WgwCfg<WCO_>;
  using R = WgwRow<ROW>;
  const int lane = tid & 63, hl = lane >> 5;
  WgwLane v;
  int cn = 0, cth = 0, ctw = 0;  // the next K-tile to stage
  if constexpr (SDMA) {
    const int pd = lane / C::D_UPX, qd = lane - pd * C::D_UPX;
    const int px = lane / X_UPX, qx = lane - px * X_UPX;
    v.vd = (unsigned)(pd * a.Cout + co0 + 4 * qd) * 4u;
    v.vx = (unsigned)(px * a.Cin + ci0 + 4 * qx) * 4u;
    v.vxl = px == 0 ? 0x80000000u : v.vx - (unsigned)a.Cin * 4u;
    int h0, w0;
    wgw_origin(a, t_beg, cn, h0, w0);
    cth = h0 / TH; ctw = w0 / TW;
  }
  auto stage = [&](int tile, float* slot) __attribute__((always_inline)) {
    if constexpr (SDMA) {
      wgw_sdma<WCO_>(a, cn, cth, ctw, wave, lane, v, slot);
      if (++ctw == a.tiles_w) {
        ctw = 0;
        if (++cth == a.tiles_h) { cth = 0; ++cn; }
      }
    } else {
      wgw_dma<WCO_>(a, tile, co0, ci0, tid, slot);
    }
  };
  if (t_beg < t_end) stage(t_beg, smem);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
  for (int tile = t_beg; tile < t_end; ++tile) {
    const int cur = (tile - t_beg) & 1;
    if (tile + 1 < t_end) stage(tile + 1, smem + (cur ^ 1) * C::SLOT);
    const float* slot = smem + cur * C::SLOT;
    const unsigned dbase = lds_addr(slot + (2 * hl) * C::DLS + 32 * cg + (lane & 31));
    const unsigned xbase = lds_addr(slot + C::D_FLOATS + R::RLO * HWD * XLS + (2 * hl) * XLS + 32 * half + (lane & 31));
    WgwOps2 ops[2];
    wgw_read2<WCO_, ROW, 0>(dbase, xbase, ops[0]);
    wgw_steps2<WCO_, ROW, 0>(dbase, xbase, ops, acc);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

template <int WCO_ = 32, bool SDMA = true>
__global__ __launch_bounds__(16 * WCO_, 1) void wgrad3x3_wino32_kernel(WgwArgs a) {
  using C = WgwCfg<WCO_>;
  __shared__ __attribute__((aligned(16))) float smem[2 * C::SLOT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = wave & 3, half = (wave >> 2) & 1, cg = wave >> 3;  // cg: 32-channel group of WCO_ = 64
  const int nmn = gridDim.x, nb = nmn * gridDim.y, id = blockIdx.y * nmn + blockIdx.x;
  const int xc = id & 7, q8 = nb >> 3, r8 = nb & 7;
  const int lb = xc * q8 + (xc < r8 ? xc : r8) + (id >> 3);
  const int mn = lb % nmn, split = lb / nmn;
  const int co0 = (mn % a.nco) * C::WCO, ci0 = (mn / a.nco) * WCI;
  const int t_beg = (int)(((long long)a.ntiles * split) / a.nsplit);
  const int t_end = (int)(((long long)a.ntiles * (split + 1)) / a.nsplit);

  f32x16 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  switch (row) {  // (wave-uniform)
    case 0: wgw_kloop<WCO_, SDMA, 0>(a, smem, t_beg, t_end, co0, ci0, tid, wave, half, cg, acc); break;
    case 1: wgw_kloop<WCO_, SDMA, 1>(a, smem, t_beg, t_end, co0, ci0, tid, wave, half, cg, acc); break;
    case 2: wgw_kloop<WCO_, SDMA, 2>(a, smem, t_beg, t_end, co0, ci0, tid, wave, half, cg, acc); break;
    default: wgw_kloop<WCO_, SDMA, 3>(a, smem, t_beg, t_end, co0, ci0, tid, wave, half, cg, acc); break;
  }

  // slab: ws[split][4*row + k][co][ci], D row = co (acc_row), col = ci (lane & 31)
  const int ci = ci0 + 32 * half + (lane & 31);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + 32 * cg + acc_row(r, lane);
      PMU_DCHECK(split < a.nsplit && co < a.Cout && ci < a.Cin, PMU_DBG_WORKSPACE);
      a.ws[(((long long)split * 16 + 4 * row + k) * a.Cout + co) * a.Cin + ci] = acc[k][r];
    }
}

// dw[co][ci][3][3] = G^T (sum over splits of M) G, G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1].
// Block = 64 consecutive (co, ci) elements x 16 components x 4 split residues (1024 threads): thread
// (q = t >> 8, comp = (t >> 4) & 15, four elements (t & 15) * 4 ...) sums splits q, q + 4, ... of its
// float4 slab column (residue 0 also the tail past the last full group of 4), the four partial sums meet
// in LDS in the fixed order (s0 + s1) + (s2 + s3) — deterministic — and 64 threads apply the output
// transform.  (16 B per load: the 4-B loads of one thread per (element, residue) kept ~1/4 of the
// bytes in flight and left the reduction latency-bound at ~21 us whatever the layer.)
__global__ __launch_bounds__(1024) void wgrad_wino_reduce_kernel(const float* __restrict__ ws, int nsplit, int Cout,
                                                                 int Cin, float* __restrict__ dw) {
  __shared__ float red[4][16][65];
  const long long CC = (long long)Cout * Cin;  // a multiple of 64 (pmu_conv3x3_wgrad_wino)
  const int q = threadIdx.x >> 8, c = (threadIdx.x >> 4) & 15, e4 = (threadIdx.x & 15) * 4;
  const long long e = (long long)blockIdx.x * 64 + e4;
  const float* p = ws + (long long)c * CC + e;
  const long long st = 16 * CC;
  const int full = nsplit >> 2;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int k = 0; k < full; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(p + (long long)(4 * k + q) * st);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  if (q == 0)
    for (int sp = 4 * full; sp < nsplit; ++sp) {
      const float4 v = *reinterpret_cast<const float4*>(p + (long long)sp * st);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  red[q][c][e4 + 0] = s.x;
  red[q][c][e4 + 1] = s.y;
  red[q][c][e4 + 2] = s.z;
  red[q][c][e4 + 3] = s.w;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int el = threadIdx.x;
  float m[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) m[k] = (red[0][k][el] + red[1][k][el]) + (red[2][k][el] + red[3][k][el]);
  float t[3][4];  // G^T M
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float h = 0.5f * (m[4 + k] + m[8 + k]);
    t[0][k] = m[k] + h;
    t[1][k] = 0.5f * (m[4 + k] - m[8 + k]);
    t[2][k] = h + m[12 + k];
  }
  float* o = dw + ((long long)blockIdx.x * 64 + el) * 9;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float h = 0.5f * (t[i][1] + t[i][2]);
    o[3 * i + 0] = t[i][0] + h;
    o[3 * i + 1] = 0.5f * (t[i][1] - t[i][2]);
    o[3 * i + 2] = h + t[i][3];
  }
}

// 64-channel blocks when Cout allows
static int wgw_wco(int Cout) { return Cout % 64 == 0 ? 64 : 32; }

void wgw_geometry(int N, int H, int W, int Cout, int Cin, WgwArgs& a) {
  a.N = N; a.H = H; a.W = W; a.Cout = Cout; a.Cin = Cin;
  a.tiles_w = pmu_cdiv(W, TW);
  a.tiles_h = pmu_cdiv(H, TH);
  a.ntiles = N * a.tiles_w * a.tiles_h;
  a.nco = Cout / wgw_wco(Cout);
  const int blocks_mn = a.nco * (Cin / WCI);
  static const int target_env = pmu_env_int("PMU_WGW_BLOCKS", 0);  // workgroups the split-K aims for (A/B)
  // one wave of workgroups: 256 of the 1024-thread 64-channel blocks (one per CU; 320 / 512 / 768
  // measured 19.2 / 13.4 / 14.2 ms vs 12.9-13.0 ms per c2 step), 512 of the 512-thread ones (two per CU)
  const int target = target_env > 0 ? target_env : (wgw_wco(Cout) == 64 ? 256 : 512);
  int s = target / blocks_mn;
  if (s < 1) s = 1;
  if (s > a.ntiles) s = a.ntiles;
  a.nsplit = s;
}

}  // namespace

extern "C" size_t pmu_conv3x3_wgrad_ws_wino(int N, int H, int W, int Cin, int Cout) {
  if (Cout % WCO != 0 || Cin % WCI != 0) return 0;
  WgwArgs a;
  wgw_geometry(N, H, W, Cout, Cin, a);
  return (size_t)a.nsplit * 16 * Cout * Cin * sizeof(float);
}

// Shapes whose K-tiles the row-split kernel stages through buffer descriptors: each operand below 2^31
// bytes, so the descriptor offsets and the out-of-range marker 0x80000000 fit.  Larger operands (and
// PMU_WGW_SDMA=0 in the experiments build, read per call: A/B and tests) take the per-lane addresses.
extern "C" int pmu_conv3x3_wgrad_wino_dma_ok(int N, int H, int W, int Cin, int Cout) {
  const long long px = (long long)N * H * W;
  return N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && 4 * px * Cin < (1LL << 31) && 4 * px * Cout < (1LL << 31);
}
static bool wgw_sdma_on(int N, int H, int W, int Cin, int Cout) {
  return pmu_conv3x3_wgrad_wino_dma_ok(N, H, W, Cin, Cout) && pmu_variant_int("PMU_WGW_SDMA", 1) != 0;
}

extern "C" int pmu_conv3x3_wgrad_wino(const float* dzt, const float* xt, int N, int H, int W, int Cout, int Cin,
                                      float* dw, float* ws, size_t ws_bytes, void* stream) {
  PMU_REQUIRE(dzt && xt && dw && ws && N > 0 && H > 0 && W > 0);
  PMU_REQUIRE(Cout % WCO == 0 && Cin % WCI == 0);
  WgwArgs a;
  a.dz = dzt; a.x = xt; a.ws = ws;
  wgw_geometry(N, H, W, Cout, Cin, a);
  PMU_REQUIRE(ws_bytes >= (size_t)a.nsplit * 16 * Cout * Cin * sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(a.nco * (Cin / WCI)), (unsigned)a.nsplit);
  if (const bool sdma = wgw_sdma_on(N, H, W, Cin, Cout); wgw_wco(Cout) == 64) {
    if (sdma) hipLaunchKernelGGL((wgrad3x3_wino32_kernel<64, true>), grid, dim3(1024), 0, st, a);
    else hipLaunchKernelGGL((wgrad3x3_wino32_kernel<64, false>), grid, dim3(1024), 0, st, a);
  } else {
    if (sdma) hipLaunchKernelGGL((wgrad3x3_wino32_kernel<32, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((wgrad3x3_wino32_kernel<32, false>), grid, dim3(NT), 0, st, a);
  }
  PMU_CHECK_LAUNCH();
  const long long CC = (long long)Cout * Cin;  // Cout % WCO, Cin % WCI: a multiple of 64
  hipLaunchKernelGGL(wgrad_wino_reduce_kernel, dim3((unsigned)(CC / 64)), dim3(1024), 0, st, (const float*)ws,
                     a.nsplit, Cout, Cin, dw);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
