// On-the-fly slice augmentation on gfx950: the warped batch gather.  One launch writes the image and the
// mask of every item of a training batch, sampling the resident padded fp64 volumes (the oblique path's,
// pmu_sample.h) through a per-item in-plane affine map plus a smooth elastic displacement (a uniform cubic
// B-spline over a G x G control grid), with a per-item gain and bias on the image.  The reference has no
// counterpart (it trains on un-augmented slices, PMU/utils/mri_dataset.py:114-143); the random parameters
// are drawn on the host (pmu_hip/augment.py), the device sees numbers only.
//
// Geometry ("Augmentation").  Item b: table row item[b][0] (volume, padded dims p, frame n u v),
// parameter block par[b] = [ds, m00, m01, m10, m11, ta, tb, gain, bias], control grid ctrl[b][2][G][G].
// Output pixel (a, b) of H x W at spacing h:
//   pa = h (a - (H-1)/2), pb = h (b - (W-1)/2);  (d0, d1) = the B-spline at (a, b), 0 when G = 0;
//   pa' = pa + d0, pb' = pb + d1;  qa = (m00 pa' + m01 pb') + ta, qb = (m10 pa' + m11 pb') + tb;
//   x_i = c_i + ((ds n_i + qa u_i) + qb v_i), c_i = (p_i - 1) / 2   (grid_to_voxel);
//   image (float)(y gain + bias), y = trilinear(x) / m (m the un-warped slice's max, when non-zero);
//   mask  (float) nearest(x).
// Everything is fp64 in this one order with FP contraction off (the pragma covers the file), so a numpy
// restatement (tests/augment_ref.py) reproduces the kernel bit for bit, and the identity block reproduces
// pmu_oblique_gather and, on the standard axes, pmu_gather_slices.
//
// Shape: one output pixel per thread; a 256-thread block owns a 16 x 16 tile of one item, so the eight
// voxel reads of neighbouring lanes stay within a small brick of the volume on any rotated plane.  The
// block stages the item's parameter block, its control grid (all of it: 2 G^2 <= 512 doubles, 4 KiB, two
// loads per thread from a line every tile of the item shares) and the tile's 16 row and 16 column weight
// quadruples in LDS once: the weights depend on a or on b only, so 32 threads compute what 256 would.
// The kernel is a latency-bound gather (nine dependent-address loads per pixel): at 5.2 KiB of LDS per block
// and 42 VGPRs the CU holds its full 8 waves per SIMD.
#include "pmu_common.h"
#include "pmu_sample.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 16;   // the block's tile edge: TILE * TILE = 256 threads
constexpr int GMAX = 16;   // largest control grid edge

struct WarpArgs {
  const long long* vaddr_img;
  const long long* vaddr_mask;
  const int* dims;
  const double* frames;
  const int* item;
  const double* maxv;
  const double* par;
  const double* ctrl;
  int nrows, G, H, W;
  double h;
  float* img_out;
  float* mask_out;
};

// cell i and the four uniform cubic B-spline weights of output index p of n along one axis of a G-point grid
__device__ __forceinline__ int spline_cell(int p, int n, int G, double* w) {
  const double u = (double)p * ((double)(G - 3) / (double)(n - 1));
  const int i = min((int)floor(u), G - 4);
  const double t = u - (double)i;
  const double omt = 1.0 - t, t2 = t * t, t3 = t2 * t;
  w[0] = ((omt * omt) * omt) / 6.0;
  w[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
  w[2] = (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0;
  w[3] = t3 / 6.0;
  return i;
}

__global__ __launch_bounds__(TILE * TILE) void warp_gather_kernel(WarpArgs a) {
  __shared__ double s_par[9];
  __shared__ double s_ctrl[2 * GMAX * GMAX];
  __shared__ double s_w[2][TILE][4];
  __shared__ int s_cell[2][TILE];
  const int tid = threadIdx.x, item = blockIdx.z;
  const int G = a.G, H = a.H, W = a.W;
  const int la = tid >> 4, lb = tid & (TILE - 1);
  if (tid < 9) s_par[tid] = a.par[9 * (long long)item + tid];
  if (G) {
    const double* c = a.ctrl + (long long)item * 2 * G * G;
    for (int e = tid; e < 2 * G * G; e += TILE * TILE) s_ctrl[e] = c[e];
    // wave 0: the tile's row weights in lanes 0..15, its column weights in lanes 16..31
    if (tid < 2 * TILE) {
      const int axis = tid >> 4;
      const int p = (axis ? blockIdx.x : blockIdx.y) * TILE + lb;
      s_cell[axis][lb] = spline_cell(p, axis ? W : H, G, s_w[axis][lb]);
    }
  }
  __syncthreads();
  const int pa_i = blockIdx.y * TILE + la, pb_i = blockIdx.x * TILE + lb;
  if (pa_i >= H || pb_i >= W) return;
  const int r = a.item[2 * item], mi = a.item[2 * item + 1];
  PMU_DCHECK(r >= 0 && r < a.nrows, PMU_DBG_INDEX);
  PMU_DCHECK(!a.maxv || mi >= 0, PMU_DBG_INDEX);
  const int p0 = a.dims[3 * r], p1 = a.dims[3 * r + 1], p2 = a.dims[3 * r + 2];
  const Frame f = load_frame(a.frames + 9 * r);
  const double pa = a.h * ((double)pa_i - (double)(H - 1) / 2.0);
  const double pb = a.h * ((double)pb_i - (double)(W - 1) / 2.0);
  double d[2] = {0.0, 0.0};
  if (G) {
    const int ia = s_cell[0][la], ib = s_cell[1][lb];
    PMU_DCHECK(ia >= 0 && ia + 3 < G && ib >= 0 && ib + 3 < G, PMU_DBG_INDEX);
    const double* wa = s_w[0][la];
    const double* wb = s_w[1][lb];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double* c = s_ctrl + (k * G + ia) * G + ib;
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double* q = c + i * G;
        const double row = ((wb[0] * q[0] + wb[1] * q[1]) + wb[2] * q[2]) + wb[3] * q[3];
        acc = i ? acc + wa[i] * row : wa[0] * row;
      }
      d[k] = acc;
    }
  }
  const double pa2 = pa + d[0], pb2 = pb + d[1];
  const double ds = s_par[0];
  const double qa = (s_par[1] * pa2 + s_par[2] * pb2) + s_par[5];
  const double qb = (s_par[3] * pa2 + s_par[4] * pb2) + s_par[6];
  const double x0 = grid_to_voxel(f, 0, (double)(p0 - 1) / 2.0, ds, qa, qb);
  const double x1 = grid_to_voxel(f, 1, (double)(p1 - 1) / 2.0, ds, qa, qb);
  const double x2 = grid_to_voxel(f, 2, (double)(p2 - 1) / 2.0, ds, qa, qb);
  const long long o = ((long long)item * H + pa_i) * W + pb_i;
  if (a.img_out) {
    PMU_DCHECK(a.vaddr_img[r] != 0, PMU_DBG_INDEX);
    const double x = sample_volume(reinterpret_cast<const double*>(a.vaddr_img[r]), p0, p1, p2, x0, x1, x2, 0);
    const double m = a.maxv ? a.maxv[mi] : 0.0;
    const double y = m != 0.0 ? x / m : x;
    a.img_out[o] = (float)(y * s_par[7] + s_par[8]);
  }
  if (a.mask_out) {
    PMU_DCHECK(a.vaddr_mask[r] != 0, PMU_DBG_INDEX);
    a.mask_out[o] = (float)sample_volume(reinterpret_cast<const double*>(a.vaddr_mask[r]), p0, p1, p2, x0, x1, x2, 1);
  }
}

}  // namespace

extern "C" int pmu_warp_gather(const long long* vaddr_img, const long long* vaddr_mask, const int* dims,
                               const double* frames, int nrows, const int* item, const double* maxv,
                               const double* par, const double* ctrl, int G, int B, int H, int W, double h,
                               float* img_out, float* mask_out, void* stream) {
  PMU_REQUIRE(vaddr_img && vaddr_mask && dims && frames && item && par && nrows > 0 && B >= 1 && B <= 65535 &&
              H >= 2 && W >= 2 && H <= 32768 && W <= 32768 && h > 0.0 && (img_out || mask_out));
  PMU_REQUIRE(G == 0 || (G >= 4 && G <= GMAX && ctrl));
  WarpArgs a{vaddr_img, vaddr_mask, dims, frames, item, maxv, par, ctrl, nrows, G, H, W, h, img_out, mask_out};
  hipLaunchKernelGGL(warp_gather_kernel, dim3((unsigned)pmu_cdiv(W, TILE), (unsigned)pmu_cdiv(H, TILE), (unsigned)B),
                     dim3(TILE * TILE), 0, (hipStream_t)stream, a);
  PMU_CHECK_LAUNCH();
  return PMU_OK;
}
