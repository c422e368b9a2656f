/*
 * pmunet_hip.h — C ABI of libpmunet_hip.so, the MI355X (gfx950) hot path of the
 * Probabilistic Multi-Planar U-Net.
 *
 * The reference (qzs634/Probabilistic-Multiplanar-Unet) has no FFI: its hot path is
 * PyTorch module code.  Each entry point below replaces the PyTorch operator(s) the
 * reference calls at the cited line (PMU/ = Probabilistic-Multiplanar-Unet/):
 *
 *   pmu_conv3x3_fwd      nn.Conv2d(3x3,pad 1)+bias, with the producer's BatchNorm2d(train/eval)
 *                        + ReLU (+MaxPool2d(2) | AvgPool2d(2,ceil) | F.pad+torch.cat) fused
 *                        into the operand load     PMU/model/unet/unet_parts.py:15-20,33,52-66
 *                                                  PMU/model/probabilistic_unet/probabilistic_unet.py:36-44
 *   pmu_conv3x3_dgrad    autograd of the above w.r.t. its input (BN-backward fused in the load)
 *   pmu_conv3x3_wgrad    autograd of the above w.r.t. its weight (split-K, deterministic)
 *   pmu_conv_first_fwd / _wgrad   the Cin<=4 first layer of UNet / prior / posterior
 *   pmu_convT2x2_fwd/_dgrad/_wgrad  nn.ConvTranspose2d(k2,s2)        unet_parts.py:52
 *   pmu_bn_*             BatchNorm2d batch statistics, running-stat update, backward coefficients
 *   pmu_maxpool2_bwd / pmu_avgpool2_bwd                              unet_parts.py:33, probabilistic_unet.py:36
 *   pmu_head1x1_fwd/_bwd, pmu_wgrad1x1   OutConv + sigmoid           unet_parts.py:70-76, unet_model.py:48-49
 *   pmu_sgd_clip         clip_grad_value_(0.1) + SGD(momentum)        PMU/train.py:65,108-110
 *   pmu_bce_* / pmu_ce_* BCELoss / CrossEntropyLoss (+ grad)          trainer/unet_trainer.py:23,30-37
 *   pmu_softdice_*       soft Dice training loss (+ grad): dice_coeff's formula, PMU/dice_loss.py:5-12, on
 *                        probabilities (the reference reports Dice, it never trains on it)
 *   pmu_boundary_*       boundary loss (+ grad) on an exact signed distance map of the target batch, formed on
 *                        the device per step (extension: Kervadec et al., MIDL 2019)
 *   pmu_dice_counts      dice_coeff + argmax/one-hot                 PMU/dice_loss.py:5-12, trainer/unet_trainer.py:39-58
 *   pmu_dice_sums        dice_coeff's three sums for arbitrary tensors PMU/dice_loss.py:5-12
 *   pmu_fcomb_*          Fcomb 1x1 chain with tiled z                 probabilistic_unet.py:116-181
 *   pmu_fcomb_stats      mean / entropy / mutual-information maps of S samples, fused into the chain (extension)
 *   pmu_label_pair_counts  label-overlap counts of the generalised energy distance (extension)
 *   pmu_surface_edt / pmu_surface_collect  exact 3-D Euclidean distance transform to a class surface and the
 *                        gather of surface distances: HD, HD95, ASSD, surface Dice (extension)
 *   pmu_cc_label / pmu_cc_compact / pmu_cc_sizes / pmu_cc_filter / pmu_cc_overlap
 *                        3-D connected components of a label volume: clean-up of the fused label map
 *                        (keep the largest components) and lesion-wise detection scores (extension)
 *   pmu_interior_edt / pmu_local_thickness  distance of a class's voxels to the nearest voxel outside it and the
 *                        covering pass over it: local thickness and volume of a structure (extension)
 *   pmu_spatial_mean(_bwd) / pmu_linear_*   AxisAlignedConvGaussian head  probabilistic_unet.py:95-108
 *   pmu_slice_view_layout / pmu_slice_max / pmu_gather_slices
 *                        MRI_Dataset pad_dimensions/sample_slice/preprocess  PMU/utils/mri_dataset.py:70-112
 *   pmu_fuse3view        eval.py 3-view volume fusion + per-class Dice PMU/eval.py:42-65,157-203
 *   pmu_oblique_slice_max / pmu_oblique_gather / pmu_fuse_oblique
 *                        the same along arbitrary view vectors         extends mri_dataset.py:60-66, eval.py:157-203
 *   pmu_fusion3_eval / pmu_fusion_oblique_eval
 *                        learned fusion of the views (per-view, per-class weights): apply, and the loss and
 *                        gradient sums of its fit                      extends eval.py:157-203
 *   pmu_warp_gather      image + mask batch through a random affine + elastic warp (extension: augmentation)
 *
 * Conventions
 *   - All tensors are device pointers, fp32, activations stored channels-last (NHWC),
 *     weights in PyTorch's native layouts ([Cout][Cin][3][3], ConvT [Cin][Cout][2][2]).
 *   - Every call is asynchronous on the given hipStream_t (passed as void*), never
 *     allocates, never synchronises, and is safe to capture in a hipGraph.
 *   - Every call returns 0 on success, PMU_ERR_ARG for an invalid argument (checked
 *     on the host before any launch), or the hipError_t of a failed launch.
 *   - Reductions are deterministic: fixed-shape partial slabs, no float atomics — except the
 *     metric counters (pmu_dice_counts, pmu_label_pair_counts, pmu_fuse3view, pmu_fuse_oblique and the counts of
 *     pmu_fusion3_eval / pmu_fusion_oblique_eval: fp64 atomics of integer values, exact) and
 *     pmu_dice_sums (fp64 atomics; exact for the 0/1 inputs the reference feeds it).  pmu_surface_edt and
 *     pmu_surface_collect use integer atomics only (surface counts, output slots): the distances are the same
 *     bits on every run, the order of the collected values is not fixed (their multiset is).  The pmu_cc_*
 *     entries use integer atomics only (atomicMin on the union-find forest, component counts and sizes): every
 *     result is an integer defined by the volume alone, the same bits on every run.  pmu_interior_edt and
 *     pmu_local_thickness use integer atomics only (a voxel count; a maximum over the bits of non-negative
 *     floats): the same bits on every run.  pmu_boundary_map uses integer atomics only (an OR of two flag bits
 *     per plane): the same bits on every run.
 */
#ifndef PMUNET_HIP_H
#define PMUNET_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PMU_ABI_VERSION 1

enum { PMU_OK = 0, PMU_ERR_ARG = 1001 };

/* How one conv-input source turns stored values into operand values. */
enum {
  PMU_SRC_RAW = 0,    /* value = x                                                    */
  PMU_SRC_BNRELU = 1, /* value = max(0, x*scale[c] + shift[c])        coef = [scale|shift]          */
  PMU_SRC_BNBWD = 2   /* value = dL/dz of BN+ReLU: g=x*(z*scale+shift>0);
                         scale*g + kx*(z-mean) + kc                   coef = [scale|shift|mean|kx|kc] */
};
enum { PMU_POOL_NONE = 0, PMU_POOL_MAX2 = 1, PMU_POOL_AVG2CEIL = 2 };
/* Storage type of a source's tensors (pmu_src.dtype bits; 0 = both fp32).  bf16 storage is what
 * torch.autocast(bfloat16) keeps a conv output in (config c5): the pre-BN z of the bf16 path. */
enum { PMU_DT_X_BF16 = 1, PMU_DT_Z_BF16 = 2 };

typedef struct pmu_src {
  const float* x;    /* NHWC [N][H][W][C]: raw values, pre-BN z, or upstream gradient */
  const float* z;    /* PMU_SRC_BNBWD: pre-BN z, same shape as x; else NULL          */
  const float* coef; /* per-channel coefficient block (see modes)                     */
  int mode, pool;
  int C, H, W;       /* stored tensor dims                                            */
  int off_h, off_w;  /* top/left offset of the (pooled) source inside the frame (F.pad) */
  int dtype;         /* PMU_DT_* bits: x / z stored as bf16 (read as fp32 exactly).  Only the
                        materialising and streaming calls take bf16 sources (pmu_frame_to_bf16,
                        pmu_frame_to_f32, pmu_head1x1_fwd, pmu_wgrad1x1); the others refuse them */
} pmu_src;

/* A conv operand: one frame of N x H x W pixels whose channels are the concatenation
 * of up to two sources (torch.cat([skip, up], 1) of unet_parts.py:66). */
typedef struct pmu_frame {
  pmu_src src[2];
  int nsrc;
  int N, H, W;
} pmu_frame;

/* ---- 3x3 convolution: direct-sum weight gradient (channel counts the Winograd weight gradient
 * does not take: Cout % 32 or Cin % 64 != 0) ------------------------------------------------ */
/* dw[Cout][Cin][3][3] = dL/dw; ws must hold pmu_conv3x3_wgrad_ws() bytes. */
size_t pmu_conv3x3_wgrad_ws(int N, int H, int W, int Cin, int Cout);
int pmu_conv3x3_wgrad(const pmu_frame* dz, const pmu_frame* act, int Cout, float* dw,
                      float* ws, size_t ws_bytes, void* stream);

/* ---- fp32 Winograd F(2x2,3x3) variant (the c2 fp32 path) ------------------------------
 * The same operators as pmu_conv3x3_fwd / _dgrad in fp32, computed as 16 per-component GEMMs of
 * transformed operands (B^T d B) and weights (G g G^T), output A^T M A: fp32 rounding differs from
 * the direct sum by ~1e-6 relative.  Weights pre-transformed by pmu_conv3x3_pack_wino ([32 output
 * rows][16 channels] blocks); part rows = pmu_conv3x3_tiles_wino() (16 x 16 pixel tiles); tee as
 * pmu_conv3x3_fwd / _dgrad. */
size_t pmu_conv3x3_packed_size_wino(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_wino(const float* w, int Cout, int Cin, int dgrad, float* wp, void* stream);
int pmu_conv3x3_tiles_wino(int N, int H, int W);
int pmu_conv3x3_fwd_wino(const pmu_frame* in, const float* wp, const float* bias, int Cout, float* z,
                         float* part, float* tee, void* stream);
int pmu_conv3x3_dgrad_wino(const pmu_frame* dz, const float* wp, int Cin, int Csplit, float* dx0, float* dx1,
                           float* tee, void* stream);
/* The same F(2x2,3x3) operators on a materialised operand in 1024-thread workgroups (16 waves, four per
 * SIMD; 64 output channels x 16 x 16 pixels per block; waves split the 16 components in halves).
 * C % 8 == 0; weights by pmu_conv3x3_pack_wino2h ([64 output rows][8 channels][16 components]);
 * part rows = pmu_conv3x3_tiles_wino2h() (16 x 16 pixel blocks). */
size_t pmu_conv3x3_packed_size_wino2h(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_wino2h(const float* w, int Cout, int Cin, int dgrad, float* wp, void* stream);
int pmu_conv3x3_tiles_wino2h(int N, int H, int W);
int pmu_conv3x3_fwd_wino2h(const float* xt, int Cin, int N, int H, int W, const float* wp, const float* bias,
                           int Cout, float* z, float* part, void* stream);
int pmu_conv3x3_dgrad_wino2h(const float* dzt, int Cout, int N, int H, int W, const float* wp, int Cin,
                             int Csplit, float* dx0, float* dx1, void* stream);
/* The input gradient fused with the BatchNorm+ReLU backward reduction of the layer that produced this
 * conv's operand (dx is that layer's da, no concat split): part[pmu_conv3x3_tiles_wino2h rows][2][Cin]
 * = (sum g, sum g*xhat), g = dx * (z*coef[c]+coef[Cin+c] > 0), xhat = (z-mean)*invstd — the sums
 * pmu_bn_bwd_reduce(dx, z, ...) computes, without reading dx back (PMU/model/unet/unet_parts.py:16-17). */
int pmu_conv3x3_dgrad_wino2h_bnr(const float* dzt, int Cout, int N, int H, int W, const float* wp, int Cin,
                                 float* dx, const float* z, const float* coef, const float* mean,
                                 const float* invstd, float* part, void* stream);
/* ---- fp32 Winograd F(4x4,3x3) on a materialised operand (images >= 32 x 32: the c2 fp32 default) --
 * Replaces the same nn.Conv2d forward / input gradient (PMU/model/unet/unet_parts.py:15,18; autograd of
 * PMU/model/unet/unet_model.py:31-54) as pmu_conv3x3_*_wino2h: 36 per-component GEMMs of
 * B^T d B (6x6 patches) and G g G^T, output A^T M A per 4x4 tile; fp32 rounding differs from the direct
 * sum by a few 1e-6 relative.  xt / dzt [N][H][W][C] fp32 with C % 8 == 0; weights pre-transformed by
 * pmu_conv3x3_pack_wino4 ([32 output rows][8 channels][36 components] blocks); part rows =
 * pmu_conv3x3_tiles_wino4() (32 x 32 pixel blocks). */
size_t pmu_conv3x3_packed_size_wino4(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_wino4(const float* w, int Cout, int Cin, int dgrad, float* wp, void* stream);
int pmu_conv3x3_tiles_wino4(int N, int H, int W);
int pmu_conv3x3_dgrad_wino4(const float* dzt, int Cout, int N, int H, int W, const float* wp, int Cin,
                            int Csplit, float* dx0, float* dx1, void* stream);
/* as pmu_conv3x3_dgrad_wino2h_bnr (part rows = pmu_conv3x3_tiles_wino4) */
int pmu_conv3x3_dgrad_wino4_bnr(const float* dzt, int Cout, int N, int H, int W, const float* wp, int Cin,
                                float* dx, const float* z, const float* coef, const float* mean,
                                const float* invstd, float* part, void* stream);
/* dw[Cout][Cin][3][3] from the teed operands dzt [N][H][W][Cout] and xt [N][H][W][Cin] (fp32), by
 * Winograd F(2x2,3x3): dw = G^T [sum over 2x2 tiles of (A dY A^T) .* (B^T X B)] G.  Cout % 32 == 0,
 * Cin % 64 == 0 (pmu_conv3x3_wgrad_ws_wino returns 0 otherwise); ws must hold that many bytes. */
size_t pmu_conv3x3_wgrad_ws_wino(int N, int H, int W, int Cin, int Cout);
int pmu_conv3x3_wgrad_wino(const float* dzt, const float* xt, int N, int H, int W, int Cout, int Cin,
                           float* dw, float* ws, size_t ws_bytes, void* stream);
/* 1 when pmu_conv3x3_wgrad_wino stages its K-tiles through buffer descriptors (each operand below 2^31
 * bytes); 0: it forms per-lane 64-bit addresses instead.  Same results either way; a host function. */
int pmu_conv3x3_wgrad_wino_dma_ok(int N, int H, int W, int Cin, int Cout);

/* ---- bf16-MFMA variants (config c5, BASELINE.json configs[4]: "... bf16") --------------
 * torch.autocast(bfloat16) arithmetic for the same operators: the operand (after the fused fp32
 * BN/ReLU/pool/concat transform) and the weights are rounded to bf16 (RNE), products are summed in
 * fp32 on v_mfma_f32_32x32x16_bf16, and every output (z, BN partials, dx, dw) stays fp32, so all
 * the fp32 BN / pool / head / optimizer kernels above consume them unchanged.
 * Weights are always pre-packed (bf16, [row block of 64][chunk of 16][tap][64][16]). */
size_t pmu_conv3x3_packed_size_bf16(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_bf16(const float* w, int Cout, int Cin, int dgrad, unsigned short* wp, void* stream);
/* rows of the fused-staging convs' BN partial sums (256-pixel tiles) */
int pmu_conv3x3_tiles(int N, int H, int W);
/* z = conv3x3(frame) + bias / dx as the direct-sum fp32 conv of pmu_hip_experiments.h (part rows =
 * pmu_conv3x3_tiles()).  tee (nullable):
 * receives the bf16 operand the kernel multiplied, [N][H][W][pad8(K channels)] as pmu_frame_to_bf16
 * would write it (padding channels untouched) — the input of pmu_conv3x3_wgrad_bf16, for free. */
int pmu_conv3x3_fwd_bf16(const pmu_frame* in, const unsigned short* wp, const float* bias, int Cout,
                         float* z, float* part, unsigned short* tee, void* stream);
int pmu_conv3x3_dgrad_bf16(const pmu_frame* dz, const unsigned short* wp, int Cin, int Csplit,
                           float* dx0, float* dx1, unsigned short* tee, void* stream);

/* The bf16-mode main path: a conv whose operand was materialised once by pmu_frame_to_bf16
 * (xt / dzt: [N][H][W][Cp] bf16, Cp % 8 == 0), weights packed per 64 output rows x 32 channels
 * (pmu_conv3x3_pack_raw).  Outputs as pmu_conv3x3_fwd / _dgrad; dgrad needs Csplit % 32 == 0 when
 * Csplit < Cin; N*H*W*Cp < 2^31. */
size_t pmu_conv3x3_packed_size_raw(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_raw(const float* w, int Cout, int Cin, int dgrad, unsigned short* wp, void* stream);
int pmu_conv3x3_fwd_raw(const unsigned short* xt, int Cp, int N, int H, int W, const unsigned short* wp,
                        const float* bias, int Cout, float* z, float* part, void* stream);
/* rows of pmu_conv3x3_fwd_raw's part[tile][2][Cout] (its pixel tiles are 256 or 512 pixels) */
int pmu_conv3x3_tiles_raw(int N, int H, int W, int Cout);
int pmu_conv3x3_dgrad_raw(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                          int Cin, int Csplit, float* dx0, float* dx1, void* stream);
/* The same convolutions with both operands staged by LDS-DMA (512-thread workgroups, 512- or
 * 1024-pixel tiles, 16-channel chunks), for maps at least 32 wide: Cp % 16 == 0, Csplit == Cin or
 * Csplit % 32 == 0 (pmu_conv3x3_dma_ok).  Weights packed by pmu_conv3x3_pack_dma (its own layout);
 * part rows = pmu_conv3x3_tiles_dma().  Launches whose operand reaches 4 GiB are split over images. */
int pmu_conv3x3_dma_ok(int H, int W, int Cp, int NOUT, int split);
int pmu_conv3x3_tiles_dma(int N, int H, int W, int Cout, int Cp);
size_t pmu_conv3x3_packed_size_dma(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_dma(const float* w, int Cout, int Cin, int dgrad, unsigned short* wp, void* stream);
int pmu_conv3x3_fwd_dma(const unsigned short* xt, int Cp, int N, int H, int W, const unsigned short* wp,
                        const float* bias, int Cout, float* z, float* part, void* stream);
int pmu_conv3x3_dgrad_dma(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                          int Cin, int Csplit, float* dx0, float* dx1, void* stream);
/* the same with a concat split (Csplit < Cin, (Cin - Csplit) % 8 == 0) that also writes dx1b, a bf16
 * (RNE) copy of dx1 [N][H][W][Cin-Csplit]: the up-sampled part's gradient is the transposed conv's
 * bf16 operand (unet_parts.py:52,66 under autocast) — no separate pmu_frame_to_bf16 pass over dx1 */
int pmu_conv3x3_dgrad_dma_x1b(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                              int Cin, int Csplit, float* dx0, float* dx1, unsigned short* dx1b, void* stream);
/* the same without the fp32 dx1 (only dx1b), plus part[tile][0][Cin] = per-tile column sums of dx
 * (part[tile][1][*] = 0; tiles = pmu_conv3x3_tiles_dma(N, H, W, Cin, Cp)): the transposed conv's bias
 * gradient (unet_parts.py:52 backward) is the sum over tiles of channels [Csplit, Cin)
 * (pmu_convT2x2_dbias_rows). */
int pmu_conv3x3_dgrad_dma_x1b_sum(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                                  int Cin, int Csplit, float* dx0, unsigned short* dx1b, float* part, void* stream);
/* dbias[c] = sum over r < R of part[r * ld + c], c < Cout, in a fixed order; ws holds
 * pmu_convT2x2_dbias_rows_ws(Cout) bytes. */
size_t pmu_convT2x2_dbias_rows_ws(int Cout);
int pmu_convT2x2_dbias_rows(const float* part, int R, long long ld, int Cout, float* dbias, float* ws, void* stream);
/* as pmu_conv3x3_dgrad_wino2h_bnr (part rows = pmu_conv3x3_tiles_dma(N, H, W, Cin, Cp)) */
int pmu_conv3x3_dgrad_dma_bnr(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                              int Cin, float* dx, const float* z, const float* coef, const float* mean,
                              const float* invstd, float* part, void* stream);
/* bf16 activation gradients (config c5, unet_parts.py:15,18 backward under torch.autocast(bfloat16),
 * whose conv backward returns dx in bf16): the four input gradients above with dx / dx0 stored as
 * bf16 (RNE) and every other output (dx1 values, dx1b, column sums, BN-backward partials) formed from
 * the rounded values.  Cin % 8 == 0, Csplit % 8 == 0.  Consumers: pmu_frame_to_bf16 (BN-backward
 * frames with a bf16 da), pmu_maxpool2_bwd_bnr_dxb, pmu_bn_bwd_reduce_dxb, pmu_conv_first_wgrad. */
int pmu_conv3x3_dgrad_dma_dxb(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                              int Cin, int Csplit, unsigned short* dx0, float* dx1, void* stream);
int pmu_conv3x3_dgrad_dma_x1b_dxb(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                                  int Cin, int Csplit, unsigned short* dx0, float* dx1, unsigned short* dx1b,
                                  void* stream);
int pmu_conv3x3_dgrad_dma_x1b_sum_dxb(const unsigned short* dzt, int Cp, int N, int H, int W,
                                      const unsigned short* wp, int Cin, int Csplit, unsigned short* dx0,
                                      unsigned short* dx1b, float* part, void* stream);
int pmu_conv3x3_dgrad_dma_bnr_dxb(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                                  int Cin, unsigned short* dx, const float* z, const float* coef, const float* mean,
                                  const float* invstd, float* part, void* stream);
/* The bf16 operand of a frame, materialised: out[N][H][W][Cpad] = bf16(frame value) (channels
 * >= C zero; Cpad % 4 == 0) — the BN+ReLU(+pool)(+concat) activation or the BN+ReLU backward dz
 * that pmu_conv3x3_wgrad_bf16 multiplies. */
int pmu_frame_to_bf16(const pmu_frame* f, int Cpad, unsigned short* out, void* stream);
/* out[N][H][W][C] = the frame's fp32 operand values (e.g. MaxPool2d of BN+ReLU, unet_parts.py:33). */
int pmu_frame_to_f32(const pmu_frame* f, float* out, void* stream);
/* the frame into the first channels of a wider NHWC tensor (output pixel stride ldo elements): the
 * skip half of an Up block's concat operand, whose other half pmu_convT2x2_fwd_ld /
 * pmu_convT2x2_fwd_dma_ldb write in place (unet_parts.py:66).  Channel counts of 4 (fp32) / 8 (bf16). */
int pmu_frame_to_f32_ld(const pmu_frame* f, float* out, int ldo, void* stream);
int pmu_frame_to_bf16_ld(const pmu_frame* f, int Cpad, unsigned short* out, int ldo, void* stream);
/* One pass over a level's BN+ReLU activation for both of its consumers (unet_parts.py:33 MaxPool2d
 * and :66 torch.cat): f is the max-pooled frame (one fp32 BNRELU source, even source dims, C a
 * power-of-two multiple of 8 up to 2048; pmu_frame_pool_skip_ok); out[N][H][W][C] receives the
 * pooled operand and skip (pixel stride ldo_skip >= C, a multiple of 8) the unpooled activation in
 * its first C channels.  Bit-identical to pmu_frame_to_* + pmu_frame_to_*_ld. */
int pmu_frame_pool_skip_ok(const pmu_frame* f);
int pmu_frame_to_bf16_pool_skip(const pmu_frame* f, unsigned short* out, unsigned short* skip, int ldo_skip,
                                void* stream);
int pmu_frame_to_f32_pool_skip(const pmu_frame* f, float* out, float* skip, int ldo_skip, void* stream);
/* dw[Cout][Cin][3][3] from dzt [N][H][W][pad8(Cout)] and xt [N][H][W][pad8(Cin)] (bf16, pad8(c) =
 * c rounded up to a multiple of 8); ws must hold pmu_conv3x3_wgrad_ws_bf16() bytes. */
size_t pmu_conv3x3_wgrad_ws_bf16(int N, int H, int W, int Cin, int Cout);
int pmu_conv3x3_wgrad_bf16(const unsigned short* dzt, const unsigned short* xt, int N, int H, int W,
                           int Cout, int Cin, float* dw, float* ws, size_t ws_bytes, void* stream);
/* The same weight gradient with both operands staged by LDS-DMA (csrc/wgrad3x3_bf16_dma.hip): a wave
 * owns a 32-co x 32-ci fragment pair and all nine taps, walks 16-pixel-wide image strips row by row
 * and keeps the three activation rows of a step in registers (one new row per step).  Maps at least
 * 16 wide (pmu_conv3x3_wgrad_dma_ok); ws holds pmu_conv3x3_wgrad_ws_bf16_dma() bytes. */
int pmu_conv3x3_wgrad_dma_ok(int N, int H, int W, int Cin, int Cout);
size_t pmu_conv3x3_wgrad_ws_bf16_dma(int N, int H, int W, int Cin, int Cout);
int pmu_conv3x3_wgrad_bf16_dma(const unsigned short* dzt, const unsigned short* xt, int N, int H, int W,
                               int Cout, int Cin, float* dw, float* ws, size_t ws_bytes, void* stream);

/* Weight gradient from materialised bf16 operands: xt [N][H][W][pad8(Cin)] (the convT input after BN+ReLU)
 * and dut [N][Hd][Wd][pad8(Cout)] (du); dbias (nullable) sums the fp32 du over the output region. */
/* The same forward / input gradient with both GEMM operands staged by LDS-DMA from materialised bf16
 * tensors: xt = the BN+ReLU operand [N][H][W][Cip] (pmu_frame_to_bf16), dut = du [N][Hd][Wd][Cop];
 * weights packed by pmu_convT2x2_pack_dma (2 * 4*Cin*Cout bytes).  Cin % 32 == 0, Cout % 32 == 0 and
 * the GEMM column count (forward 4*Cout, dgrad Cin) % 128 == 0 (pmu_convT2x2_dma_ok). */
int pmu_convT2x2_dma_ok(int Cin, int Cout, int dgrad);
size_t pmu_convT2x2_packed_size_dma(int Cin, int Cout);
int pmu_convT2x2_pack_dma(const float* w, int Cin, int Cout, int dgrad, unsigned short* wp, void* stream);
int pmu_convT2x2_fwd_dma(const unsigned short* xt, int Cip, int N, int H, int W, const unsigned short* wp,
                         const float* bias, int Cin, int Cout, float* u, void* stream);
/* the same written as bf16 into channels [0, Cout) of a wider NHWC bf16 tensor (pixel stride ldo):
 * the up-sampled half of the Up block's bf16 concat operand — no fp32 u (unet_parts.py:52,66) */
int pmu_convT2x2_fwd_dma_ldb(const unsigned short* xt, int Cip, int N, int H, int W, const unsigned short* wp,
                             const float* bias, int Cin, int Cout, unsigned short* ub, int ldo, void* stream);
int pmu_convT2x2_dgrad_dma(const unsigned short* dut, int Cop, int Hd, int Wd, int off_h, int off_w,
                           const unsigned short* wp, int N, int H, int W, int Cin, int Cout, float* dx,
                           void* stream);
/* the same with dx stored as bf16 (RNE; autocast's dtype for ConvTranspose2d's input gradient,
 * unet_parts.py:52 backward): its consumer's BN backward reads it (pmu_bn_bwd_reduce_dxb and the
 * BN-backward frames) */
int pmu_convT2x2_dgrad_dma_dxb(const unsigned short* dut, int Cop, int Hd, int Wd, int off_h, int off_w,
                               const unsigned short* wp, int N, int H, int W, int Cin, int Cout, unsigned short* dx,
                               void* stream);
size_t pmu_convT2x2_wgrad_ws_bf16(int N, int H, int W, int Cin, int Cout);
int pmu_convT2x2_wgrad_bf16(const unsigned short* xt, const unsigned short* dut, const float* du, int N, int H,
                            int W, int Hd, int Wd, int off_h, int off_w, int Cin, int Cout, float* dw,
                            float* dbias, float* ws, size_t ws_bytes, void* stream);

/* ---- first layer (Cin <= 4, planes given NCHW-style, one pointer per channel) ------ */
int pmu_conv_first_fwd(const float* const* planes, int Cin, int N, int H, int W,
                       const float* w, const float* bias, int Cout, float* z, float* part,
                       void* stream);
int pmu_conv_first_tiles(int N, int H, int W);
size_t pmu_conv_first_wgrad_ws(int N, int H, int W, int Cin, int Cout);
/* dz: one BN-backward (or raw) source; its da may be bf16-stored (a *_dxb input gradient's dx) */
int pmu_conv_first_wgrad(const pmu_frame* dz, const float* const* planes, int Cin, int Cout,
                         float* dw, float* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm2d ------------------------------------------------------------------- */
/* Column reduction of fp32 partials part[R][Wd] into fp64 partials out[G][Wd]. */
int pmu_colsum_f64(const float* part, int R, int Wd, double* out, int G, void* stream);
int pmu_colsum_groups(int R);
/* From fp64 sums acc[G][2][C] (sum, sumsq) over count elements: mean, invstd, coef=[scale|shift];
 * update running stats (unbiased var, momentum) when running_mean != NULL, and add 1 to
 * *num_batches_tracked when it is non-NULL (BatchNorm2d's counter, PMU/model/unet/unet_parts.py:16,19:
 * one launch instead of a separate increment per layer). */
int pmu_bn_fwd_finalize(const double* acc, int G, int C, double count, const float* gamma,
                        const float* beta, float eps, float momentum, float* running_mean,
                        float* running_var, long long* num_batches_tracked, float* mean, float* invstd,
                        float* coef, void* stream);
/* Eval mode: coef from running stats. */
int pmu_bn_eval_coef(const float* running_mean, const float* running_var, const float* gamma,
                     const float* beta, float eps, int C, float* coef, void* stream);
/* BN+ReLU backward reduction over da (NHWC) and z: part[tile][2][C] = (sum g, sum g*xhat). */
int pmu_bn_bwd_reduce(const float* da, const float* z, const float* coef, const float* mean,
                      const float* invstd, int P, int C, float* part, void* stream);
/* the same with da stored as bf16 (a *_dxb input gradient's dx); C % 4 == 0 */
int pmu_bn_bwd_reduce_dxb(const unsigned short* da, const float* z, const float* coef, const float* mean,
                          const float* invstd, int P, int C, float* part, void* stream);
int pmu_bn_bwd_tiles(int P, int C);
/* From acc[G][2][C]: dgamma, dbeta, dbias(conv bias feeding BN) and the BNBWD coef block
 * [scale|shift|mean|kx|kc]. */
int pmu_bn_bwd_finalize(const double* acc, int G, int C, double count, const float* gamma,
                        const float* coef, const float* mean, const float* invstd, float* dgamma,
                        float* dbeta, float* dbias, float* bcoef, void* stream);

/* out[P][C] = max(0, z*scale+shift) (NHWC), coef = [scale|shift]; any C (float4 path when C % 4 == 0). */
int pmu_bnrelu_apply(const float* z, const float* coef, long long P, int C, float* out, void* stream);

/* ---- pooling backward ------------------------------------------------------------ */
/* dx[N][H][W][C] += dpool routed to the first max (row-major) of each 2x2 window of
 * relu(z*scale+shift), or of z itself when coef is NULL (a standalone Down block's raw input).
 * accumulate=0 overwrites dx (zeros outside windows). */
int pmu_maxpool2_bwd(const float* dpool, const float* z, const float* coef, int N, int H, int W,
                     int C, float* dx, int accumulate, void* stream);
/* pmu_maxpool2_bwd (BN+ReLU coef, C % 4 == 0) fused with the BatchNorm+ReLU backward reduction of
 * the pooled layer over the resulting dx (= that layer's da; replaces pmu_bn_bwd_reduce for it):
 * part[pmu_maxpool2_bwd_bnr_tiles rows][2][C] = (sum g, sum g*xhat), g = dx*(z*scale+shift > 0),
 * xhat = (z-mean)*invstd.  MaxPool2d(2) backward, unet_parts.py:33; BN backward, unet_parts.py:16,19. */
int pmu_maxpool2_bwd_bnr_tiles(int N, int H, int W, int C);
int pmu_maxpool2_bwd_bnr(const float* dpool, const float* z, const float* coef, const float* mean,
                         const float* invstd, int N, int H, int W, int C, float* dx, int accumulate,
                         float* part, void* stream);
/* the same with dpool and the skip gradient stored as bf16 (the *_dxb input gradients' dx; skip
 * nullable = no accumulation): dx (fp32, a separate tensor) = skip + routed dpool, summed in fp32 as
 * autograd accumulates the skip activation's two gradients (unet_parts.py:33,66) */
int pmu_maxpool2_bwd_bnr_dxb(const unsigned short* dpool, const unsigned short* skip, const float* z,
                             const float* coef, const float* mean, const float* invstd, int N, int H, int W, int C,
                             float* dx, float* part, void* stream);
/* The pooled layer's da = skip + routed dpool kept in registers instead of stored (config c5's skip
 * levels): _stats_dxb forms only the partial sums above (bit-equal part); _bnbwd_dxb, given that
 * layer's BN-backward coefficients (pmu_bn_bwd_finalize's bcoef) and its forward coef (the routing's
 * argmax), writes dz = BN+ReLU backward of that da as the bf16 operand [N][H][W][ldo] of its input and
 * weight gradients — bit-equal to pmu_frame_to_bf16 of Src(da, BNBWD) over the stored da.  ldo == C;
 * C / 4 divides 256 or is a multiple of it. */
int pmu_maxpool2_bwd_bnr_stats_dxb(const unsigned short* dpool, const unsigned short* skip, const float* z,
                                   const float* coef, const float* mean, const float* invstd, int N, int H, int W,
                                   int C, float* part, void* stream);
int pmu_maxpool2_bwd_bnbwd_dxb(const unsigned short* dpool, const unsigned short* skip, const float* z,
                               const float* coef, const float* bcoef, int N, int H, int W, int C, int ldo,
                               unsigned short* dz, void* stream);
/* The same for fp32 dpool / skip gradients (config c2) with an fp32 dz: bit-equal to pmu_maxpool2_bwd_bnr
 * accumulating into skip and to pmu_frame_to_f32 of Src(that da, BNBWD, bcoef, z). */
int pmu_maxpool2_bwd_bnr_stats(const float* dpool, const float* skip, const float* z, const float* coef,
                               const float* mean, const float* invstd, int N, int H, int W, int C, float* part,
                               void* stream);
int pmu_maxpool2_bwd_bnbwd(const float* dpool, const float* skip, const float* z, const float* coef,
                           const float* bcoef, int N, int H, int W, int C, int ldo, float* dz, void* stream);
/* AvgPool2d(2,2,ceil_mode=True) backward: dx = dpool/count(window), overwrite. */
int pmu_avgpool2_bwd(const float* dpool, int N, int H, int W, int C, float* dx, void* stream);
/* The same (bit-equal dx, here da: N x H x W x C at the pooled layer's resolution) fused with the BN+ReLU
 * backward partial sums of the layer whose activation was pooled (probabilistic_unet.py:36 AvgPool2d,
 * :30-32 BN+ReLU): part[pmu_bn_bwd_tiles(N*H*W, C) rows][2][C] as pmu_bn_bwd_reduce forms them from
 * (da, z).  C % 4 == 0. */
int pmu_avgpool2_bwd_bnr(const float* dpool, const float* z, const float* coef, const float* mean,
                         const float* invstd, int N, int H, int W, int C, float* da, float* part, void* stream);

/* ---- ConvTranspose2d(k=2, s=2) ---------------------------------------------------- */
/* Optional packed weights (wp, pmu_convT2x2_packed_size bytes): k-contiguous B operands for the
 * pipelined GEMMs (dgrad=0: [ab][co][ci] for the forward, dgrad=1: [ci][ab][co] for dgrad). */
size_t pmu_convT2x2_packed_size(int Cin, int Cout);
int pmu_convT2x2_pack(const float* w, int Cin, int Cout, int dgrad, float* wp, void* stream);
/* u[N][2H][2W][Cout] = convT(act(frame)) + bias, frame is N x H x W x Cin.  wp (nullable) = packed
 * forward weights; used when the frame is one unpooled BN+ReLU source and Cin%16 == Cout%32 == 0. */
int pmu_convT2x2_fwd(const pmu_frame* in, const float* w, const float* wp, const float* bias, int Cout,
                     float* u, void* stream);
/* the same into channels [0, Cout) of a wider NHWC tensor (pixel stride ldo floats), the up-sampled
 * half of the Up block's fp32 concat operand; pipelined path only (wp given, pmu_convT2x2_fwd_ld_ok) */
int pmu_convT2x2_fwd_ld_ok(const pmu_frame* in, int Cout);
int pmu_convT2x2_fwd_ld(const pmu_frame* in, const float* w, const float* wp, const float* bias, int Cout,
                        float* u, int ldo, void* stream);
/* dx[N][H][W][Cin] from du (NHWC [N][Hd][Wd][Cout], convT output placed at (off_h,off_w)). */
int pmu_convT2x2_dgrad(const float* du, int Hd, int Wd, int off_h, int off_w, const float* w,
                       const float* wp, int N, int H, int W, int Cin, int Cout, float* dx, void* stream);
size_t pmu_convT2x2_wgrad_ws(int N, int H, int W, int Cin, int Cout);
int pmu_convT2x2_wgrad(const float* du, int Hd, int Wd, int off_h, int off_w,
                       const pmu_frame* act, int Cout, float* dw, float* dbias, float* ws,
                       size_t ws_bytes, void* stream);

/* ---- 1x1 head (OutConv) -------------------------------------------------------------- */
/* y[N][K][H][W] (NCHW) = w[K][C] . act(frame) + b; sigmoid applied when do_sigmoid. */
int pmu_head1x1_fwd(const pmu_frame* in, const float* w, const float* b, int K, int do_sigmoid,
                    float* y, void* stream);
/* dl = dy * s*(1-s) (do_sigmoid) or dy; da[N][H][W][C] = w^T dl (NHWC); dl written (NCHW). */
int pmu_head1x1_bwd(const float* dy, const float* y, int do_sigmoid, const float* w, int K, int C,
                    int N, int H, int W, float* dl, float* da, void* stream);
/* pmu_head1x1_bwd fused with the BatchNorm+ReLU backward reduction of the layer feeding the head
 * (da is its gradient; replaces pmu_bn_bwd_reduce for it): part[pmu_head1x1_bwd_tiles rows][2][C]
 * as pmu_maxpool2_bwd_bnr.  With dw non-NULL the same pass also forms the head's weight gradient
 * (pmu_wgrad1x1's dw[K][C] and db[K] from act = relu(z*scale+shift); ws of pmu_wgrad1x1_ws bytes) and
 * dl is not written (may be NULL).  Shapes: pmu_head1x1_bwd_bnr_ok (C = 4q, q a power of two <= 64).
 * OutConv backward, unet_parts.py:70-76; BN backward of the last DoubleConv, unet_parts.py:19. */
int pmu_head1x1_bwd_bnr_ok(int N, int H, int W, int C);
int pmu_head1x1_bwd_tiles(int N, int H, int W);
int pmu_head1x1_bwd_bnr(const float* dy, const float* y, int do_sigmoid, const float* w, int K, int C,
                        int N, int H, int W, float* dl, float* da, const float* z, const float* coef,
                        const float* mean, const float* invstd, float* part, float* dw, float* db, float* ws,
                        size_t ws_bytes, void* stream);
/* With dw non-NULL, da may be NULL too (not stored): pmu_head1x1_bwd_dz then writes the last layer's
 * dz straight from dy — da = sum_k g_k w[k] formed as the pass above forms it — as that layer's
 * BN+ReLU backward over bcoef (pmu_bn_bwd_finalize's 5 C coefficients): bf16 bits (out_bf16, C % 8
 * == 0; the bf16 convs' operand) or fp32, [N][H][W][C]; bit-equal to pmu_frame_to_bf16 / _f32 of
 * Src(stored da, BNBWD, bcoef, z).  Shapes as pmu_head1x1_bwd_bnr_ok, K <= 8. */
int pmu_head1x1_bwd_dz(const float* dy, const float* y, int do_sigmoid, const float* w, int K, int C,
                       int N, int H, int W, const float* z, const float* bcoef, int out_bf16, void* dz,
                       void* stream);
size_t pmu_wgrad1x1_ws(int P, int K, int C);
/* dw[K][C] = sum_p dl[p][k] act[p][c], db[k] = sum_p dl[p][k]; dl NCHW [N][K][H][W]. */
int pmu_wgrad1x1(const float* dl, const pmu_frame* act, int K, float* dw, float* db, float* ws,
                 size_t ws_bytes, void* stream);

/* ---- optimizer --------------------------------------------------------------------- */
/* Multi-tensor fused clip_grad_value_ + SGD(momentum, dampening 0, no nesterov):
 *   g = clamp(gscale*g, -clip, clip) (clip <= 0: no clipping); buf = momentum*buf + g; p -= lr*buf.
 * (buf starting at zero reproduces torch's first-step buf = g; gscale = 1/world_size turns an
 * all-reduced gradient sum into the data-parallel mean before clipping.)
 * ptrs: device array of 3*ntensors pointers (p, g, buf); chunks: device array, one block each. */
typedef struct pmu_sgd_chunk {
  int tensor; /* index into ptrs/3 */
  int len;    /* elements in this chunk (any; 16-B aligned chunks of 16384 stream float4) */
  long long start;
} pmu_sgd_chunk;
int pmu_sgd_clip(const pmu_sgd_chunk* chunks, int nchunks, void* const* ptrs, float gscale, float lr,
                 float momentum, float clip, void* stream);

/* ---- losses (row a6) -------------------------------------------------------------------
 * nn.BCELoss on the sigmoid head / nn.CrossEntropyLoss on the logits (PMU/trainer/unet_trainer.py:
 * 23,30-37) and the summed CE of ProbabilisticUnet.elbo (probabilistic_unet.py:286-304).
 * reduction: 0 none (loss[i] per element / pixel), 1 mean, 2 sum (loss[0]).  Forward partial sums
 * are fp64 in a fixed order (deterministic); ws: pmu_loss_ws(n) bytes (n = elements / pixels).
 * count_out (optional, device float): the mean's denominator (n for BCE, non-ignored pixels for
 * CE), read by pmu_ce_bwd for reduction 1.  Backward: gout is the upstream gradient on the device
 * (a scalar for mean/sum, per element for none); BCE dy = g (y - t) / max(y (1 - y), 1e-12) (torch's
 * formula; mean divides g by n); CE dx = g (softmax - onehot(t)), ignore_index pixels 0.
 * Logits x NCHW [N][K][HW], targets int64 [N][HW]. */
size_t pmu_loss_ws(long long n);
int pmu_bce_fwd(const float* y, const float* t, long long n, int reduction, float* loss, double* ws,
                float* count_out, void* stream);
int pmu_bce_bwd(const float* y, const float* t, long long n, int reduction, const float* gout, float* dy,
                void* stream);
int pmu_ce_fwd(const float* x, const long long* tgt, int N, int K, long long HW, int reduction,
               long long ignore_index, float* loss, double* ws, float* count_out, void* stream);
int pmu_ce_bwd(const float* x, const long long* tgt, int N, int K, long long HW, int reduction,
               long long ignore_index, const float* gout, const float* count, float* dx, void* stream);

/* ---- soft Dice training loss (row a6) ------------------------------------------------------
 * loss = 1 - mean D, D = (2 I + eps) / (P + T + eps) with dice_coeff's formula and smoothing
 * (PMU/dice_loss.py:5-12, eps = 1e-6), on probabilities instead of hard labels.  The reference only
 * reports Dice; differentiating it is the north star's (BASELINE.json: "a wavefront-reduced
 * dice_loss.py", KL+Dice), not the reference's.
 * K >= 2: x NCHW logits [N][K][HW], p = softmax over K, tgt int64 [N][HW]; pixels with tgt ==
 * ignore_index are left out; a target outside [0, K) gives a NaN loss and a NaN gradient at that pixel.
 * K == 1: x [N][HW] a probability (act 0) or a logit (act 1: sigmoid in the kernel), tgt a float mask
 * [N][HW] used by value.  K <= 8.  I = sum p [t = k], P = sum p, T = sum [t = k] (K == 1: sum p t, sum
 * p, sum t) over the batch (per_image 0, dice_coeff's pooling) or per image (per_image 1); the mean runs
 * over the classes first_class (0 or 1; 1 drops the background; K == 1: always 0) .. K - 1 and, per
 * image, the images: M terms.  Sums are fp64 in a fixed order (deterministic, no atomics).
 * ws: pmu_softdice_ws(N, K, HW) bytes, 8-byte aligned.  After pmu_softdice_fwd it begins with the
 * backward's coefficients coef[R][K][2] (fp32; R = N per image, else 1): a = 2 / (M S), b = (2 I + eps) /
 * (M S^2), S = P + T + eps, both 0 for a class left out; the fp64 sums [R][3K + 1] (I, P, T per class,
 * then the count of out-of-range targets) and the per-block partials follow.
 * Backward: coef = the start of the forward's ws; gout the upstream gradient, a device scalar;
 * c_k = b_k - a_k [t = k];  K >= 2: dx_j = g p_j (c_j - sum_k p_k c_k);  act 1: dx = g c p (1 - p);
 * act 0: dx = g c (c = b - a t); ignored pixels 0. */
size_t pmu_softdice_ws(int N, int K, long long HW);
int pmu_softdice_fwd(const float* x, const void* tgt, int N, int K, long long HW, int act, int per_image,
                     int first_class, long long ignore_index, float* loss, void* ws, void* stream);
int pmu_softdice_bwd(const float* x, const void* tgt, int N, int K, long long HW, int act, int per_image,
                     long long ignore_index, const float* coef, const float* gout, float* dx, void* stream);

/* ---- boundary loss (extension: Kervadec et al., MIDL 2019, on a signed distance map formed on the device) ----
 * x (N, K, H, W) fp32; the target int64 class indices [N][H][W] for K >= 2 (kind 0) or a float mask [N][H][W]
 * for K == 1 (kind 1).  Bounds: 1 <= H, W <= PMU_SURFACE_MAX_DIM, 1 <= K <= 8, N <= 65535; distances in pixels.
 *
 * Membership.  K >= 2: pixel q of image n belongs to class k iff t(n, q) == k; a pixel with t == ignore_index
 * belongs to no class (so does any other value outside [0, K)).  K == 1: q is a member iff t(n, q) >= 0.5.
 *
 * Signed map phi(n, k, .).  If the plane has no member, or no non-member, phi = 0 on that plane.  Otherwise
 *     for a non-member q   phi(q) = sqrt_rn(min over members r of |q - r|^2),
 *     for a member q       phi(q) = 1 - sqrt_rn(min over non-members r of |q - r|^2);
 * positions outside the image are not seeds.  This is one_hot2dist of the paper's code,
 * edt(neg) * neg - (edt(pos) - 1) * pos.  Squared distances are integers below 2^24, exact in fp32; with the
 * correctly rounded fp32 square root and one fp32 subtraction the map is a pure function of the target, bit-equal
 * to the numpy restatement tests/boundary_ref.py.
 *
 * Loss.  v(n, q) = 1 unless the pixel is ignored (K == 1: every pixel is valid).  The classes run over
 * k = first_class .. K - 1 (first_class 0 or 1; K == 1: the one class).  p = softmax over all K logits for K >= 2;
 * K == 1: p = x (act 0) or sigmoid(x) (act 1).  cnt = (number of valid pixels) (K - first_class),
 *     L = (1 / cnt) sum v p_k phi_k,      L = 0 when cnt == 0.   L may be negative.
 * Gradient, g the upstream scalar:  K >= 2: dx_j = (g / cnt) v p_j ([j >= first_class] phi_j - sum_{k >= first_class}
 * p_k phi_k);  act 0: dx = g phi / cnt;  act 1: dx = g phi p (1 - p) / cnt.
 *
 * pmu_boundary_ws: bytes of the workspace of pmu_boundary_map and pmu_boundary_fwd for such a batch (0 for a shape
 * outside the bounds), 8-byte aligned: the forward's per-block partial sums, then one flag word per plane and one
 * membership bit per pixel and class.  One buffer serves both calls.
 * pmu_boundary_map: writes phi [N][K][H][W].  The target is read once; the row distances are rebuilt from the
 * membership bits inside the column pass, so phi is the only other write; the absent / full test of a plane is a
 * flag pair reduced on the device (integer atomics).  The same bits on every run.
 * pmu_boundary_fwd: loss[0] = L and count[0] = cnt (a device double, read by the backward): fp32 softmax, fp64
 * products and sums in a fixed order, no float atomics — bit-identical runs.  tgt may be null for K == 1.
 * pmu_boundary_bwd: one elementwise pass scaled on the device by gout[0] / count[0]; ignored pixels 0.
 * Nothing synchronises with the host. */
size_t pmu_boundary_ws(int N, int K, int H, int W);
int pmu_boundary_map(const void* tgt, int kind, int N, int K, int H, int W, long long ignore_index, float* phi,
                     void* ws, void* stream);
int pmu_boundary_fwd(const float* x, const void* tgt, const float* phi, int N, int K, long long HW, int act,
                     int first_class, long long ignore_index, float* loss, double* count, void* ws, void* stream);
int pmu_boundary_bwd(const float* x, const void* tgt, const float* phi, int N, int K, long long HW, int act,
                     int first_class, long long ignore_index, const float* gout, const double* count, float* dx,
                     void* stream);

/* ---- metrics ------------------------------------------------------------------------- */
/* counts[k][3] = (sum pred_k*t_k, sum pred_k, sum t_k) for k < K, exact (integer-valued fp64).
 * K==1: pred = (y > 0.5), t = mask.  K>1: pred = onehot(first argmax_c softmax(y)), t = (mask == k).
 * y NCHW [N][K][H][W], mask [N][H][W]. */
int pmu_dice_counts(const float* y, const float* mask, int N, int K, int H, int W,
                    double* counts, void* stream);
/* pmu_dice_counts of S predictions y[S][N][K][H][W] against one mask in one launch: counts[S][K][3],
 * the same integers as S pmu_dice_counts calls (the eval over several prior samples,
 * PMU/trainer/probunet_trainer.py:41-60). */
int pmu_dice_counts_many(const float* y, const float* mask, int S, int N, int K, int H, int W, double* counts,
                         void* stream);

/* (sum a*b, sum a, sum b) over n elements into out[3] (fp64): dice_coeff's three sums
 * (PMU/dice_loss.py:5-12) for arbitrary pred/target tensors. */
int pmu_dice_sums(const float* a, const float* b, long long n, double* out, void* stream);

/* Pairwise label overlaps for the generalised energy distance.  maps [R][N][HW] u8: R label maps of the
 * same N images (S sample maps, then the ground truths).  inter[n][i][j][c] = pixels with maps[i] == c and
 * maps[j] == c ([N][R][R][K], symmetric, diagonal = cnt), cnt[n][i][c] = pixels with maps[i] == c
 * ([N][R][K]): exact (integer-valued fp64, the same on every run), overwritten.  Labels >= K count nowhere.
 * Bounds: R <= 64, K <= 32, N <= 65535, HW < 2^31 and R(R+1)/2 * K <= PMU_LABEL_PAIRS_MAX_COUNTERS (a
 * block keeps one 32-bit counter per (pair, class) in LDS: 32 KiB); otherwise PMU_ERR_ARG. */
#define PMU_LABEL_PAIRS_MAX_COUNTERS 8192
int pmu_label_pair_counts(const unsigned char* maps, int R, int N, long long HW, int K, double* inter,
                          double* cnt, void* stream);

/* ---- surface distances (extension: HD, HD95, ASSD and surface Dice of a label volume) -----------
 * lab [D0][D1][D2] u8.  The surface of class cls is every voxel labelled cls with at least one of its six
 * face neighbours not labelled cls; a neighbour outside the volume counts as not cls (mask ^
 * binary_erosion(mask), 6-connected, border value 0).  The squared distance of an index difference
 * (e0, e1, e2) under fp32 voxel sizes (s0, s1, s2) is defined in fp32, every operation rounded once:
 *     t_i = fl(fl(s_i * float(e_i)) * fl(s_i * float(e_i))),    d2 = fl(fl(t_2 + t_1) + t_0).
 *
 * pmu_surface_edt: d2[v] = the minimum of that squared distance over the surface voxels of cls (+inf
 * everywhere when there are none), an exact Euclidean distance transform: three separable in-place passes
 * (axis 2, 1, 0) whose result is bit-equal to the brute-force minimum.  *n_surface (a device word) = the
 * number of surface voxels.  Both are overwritten.
 * pmu_surface_collect: appends d2_other[v] to out for every surface voxel v of cls in lab, in unspecified
 * order (the multiset is the result; the caller sorts); *n_out (a device word) = the number of surface
 * voxels.  At most cap values are written: with a larger surface nothing is written beyond out[cap - 1] and
 * *n_out still reports the full count.
 * Bounds: 1 <= D0, D1, D2 <= PMU_SURFACE_MAX_DIM (a line by a tile of columns is staged in LDS),
 * D0 * D1 * D2 < 2^31, 0 <= cls <= 255, voxel sizes finite and positive, cap >= 0, pointers non-null (out
 * may be null when cap is 0); otherwise PMU_ERR_ARG.  The counters are integer atomics: every run gives the
 * same d2, the same counts and the same multiset. */
#define PMU_SURFACE_MAX_DIM 1024
int pmu_surface_edt(const unsigned char* lab, int D0, int D1, int D2, int cls, float s0, float s1, float s2,
                    float* d2, unsigned long long* n_surface, void* stream);
int pmu_surface_collect(const unsigned char* lab, int D0, int D1, int D2, int cls, const float* d2_other,
                        float* out, long long cap, unsigned long long* n_out, void* stream);

/* ---- local thickness (extension: thickness and volume of a segmented structure) -----------------
 * With lab, cls, the voxel sizes and the fp32 squared distance d2(p, q) of pmu_surface_edt:
 *
 * pmu_interior_edt: for a voxel p labelled cls, d2[p] = the minimum of d2(p, q) over all positions q not labelled
 * cls, a position outside the volume counting as not cls (the border rule of the surface); for every other
 * voxel d2[p] = 0.  Every voxel of the class gets a finite positive value.  The separable passes of
 * pmu_surface_edt seeded with the voxels off the class, then one elementwise minimum with the border term
 * min_i t_i(min(p_i + 1, D_i - p_i)) (the nearest position outside the volume lies straight out along one
 * axis); bit-equal to the brute-force minimum over the volume padded by one voxel.  *n_voxels (a device word)
 * = the number of voxels labelled cls.  Both are overwritten.
 *
 * pmu_local_thickness: takes such a field (a voxel belongs to the structure where d2 > 0) and writes
 *     r2[p] = max{ d2[q] : d2[q] > 0, d2(p, q) < d2[q] }   where d2[p] > 0,   0 elsewhere:
 * the squared radius of the largest open ball, centred on a voxel and holding voxels of the structure only, that
 * contains p (Hildebrand & Ruegsegger's local thickness is 2 sqrt(r2)).  The inequality is strict: the nearest
 * outside position of q lies at exactly d2[q].  r2 >= d2 everywhere.  A tiled exact search: a workgroup owns a
 * tile of PMU_THICKNESS_TILE^3 output voxels and walks the source tiles within reach of the field's maximum,
 * skipping those that cannot raise any of its voxels (csrc/thickness.hip).  r2 must not alias d2.
 * ws: scratch of at least pmu_local_thickness_ws(D0, D1, D2) bytes (0 for a shape outside the bounds), 4-byte
 * aligned, overwritten: the field's maximum and one maximum per tile.  Nothing is read back by the host.
 *
 * Bounds: as pmu_surface_edt — 1 <= D0, D1, D2 <= PMU_SURFACE_MAX_DIM, D0 * D1 * D2 < 2^31, 0 <= cls <= 255,
 * voxel sizes finite and positive, pointers non-null, ws_bytes large enough; otherwise PMU_ERR_ARG and nothing
 * is launched.  The field is expected finite and non-negative (what pmu_interior_edt writes); a value that is
 * not positive counts as 0.  Integer atomics only: every run gives the same bits. */
#define PMU_THICKNESS_TILE 8
int pmu_interior_edt(const unsigned char* lab, int D0, int D1, int D2, int cls, float s0, float s1, float s2,
                     float* d2, unsigned long long* n_voxels, void* stream);
size_t pmu_local_thickness_ws(int D0, int D1, int D2);
int pmu_local_thickness(const float* d2, int D0, int D1, int D2, float s0, float s1, float s2, float* r2, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- connected components (extension: clean-up of label volumes, lesion-wise detection scores) ----
 * lab [D0][D1][D2] u8, V = D0 * D1 * D2 voxels.  Value 0 is background and belongs to no component.  Two
 * voxels are adjacent under connectivity 6 (faces), 18 (faces and edges) or 26 (faces, edges and corners);
 * they are in one component when a chain of adjacent voxels of the same non-zero value joins them (different
 * values never merge).
 *
 * pmu_cc_ws: workspace bytes of pmu_cc_label and pmu_cc_compact for such a volume (0 for a shape outside
 * the bounds).  One buffer serves both calls: the compact pass keeps its per-block counts there, the
 * labelling keeps its forest in root and checks the size only.
 * pmu_cc_label: root[v] = 0 where lab[v] == 0, otherwise 1 + the smallest linear index of v's component;
 * *n_components (a device word) = the number of components.  A union-find whose forest lives in root: a merge
 * inside each workgroup's tile in LDS, a merge across tile faces in global memory (atomicMin, relaxed
 * agent-scope accesses only), a flatten pass — three launches fixed by the shape, no kernel waits on another
 * workgroup, nothing is read back.
 * pmu_cc_compact: ids[v] = the rank (1..n) of root[v] among the distinct non-zero roots in ascending order
 * (the numbering of scipy.ndimage.label: raster order of each component's first voxel), 0 for background;
 * *n (a device word) = the number of components.  Reduce-then-scan over the flags root[v] == v + 1.  ids may
 * alias root.
 * pmu_cc_sizes: size[i-1] = the voxel count of component i, cls[i-1] = its label value.
 * pmu_cc_filter: out[v] = lab[v] where ids[v] != 0 and keep[ids[v]-1] != 0, otherwise 0.  out may alias lab.
 * pmu_cc_overlap: hit_a[i-1] = 1 when some voxel v of component i of volume a has lab_b[v] == lab_a[v] (it
 * touches the same class in b), otherwise 0; hit_b likewise.
 * Every output is overwritten.  Bounds: 1 <= D0, D1, D2 <= PMU_CC_MAX_DIM, V < 2^31 (1 + an index fits an
 * int), connectivity 6, 18 or 26, 0 <= n <= V, ws_bytes >= pmu_cc_ws of the volume, pointers non-null (the
 * per-component arrays size, cls, keep, hit_a, hit_b may be null when their n is 0); otherwise PMU_ERR_ARG.
 * All counters are integer atomics: every run gives identical results. */
#define PMU_CC_MAX_DIM 1024
size_t pmu_cc_ws(int D0, int D1, int D2);
int pmu_cc_label(const unsigned char* lab, int D0, int D1, int D2, int connectivity, int* root,
                 unsigned long long* n_components, void* ws, size_t ws_bytes, void* stream);
int pmu_cc_compact(const int* root, long long V, int* ids, unsigned long long* n, void* ws, size_t ws_bytes,
                   void* stream);
int pmu_cc_sizes(const int* ids, const unsigned char* lab, long long V, long long n, long long* size,
                 unsigned char* cls, void* stream);
int pmu_cc_filter(const unsigned char* lab, const int* ids, long long V, const unsigned char* keep, long long n,
                  unsigned char* out, void* stream);
int pmu_cc_overlap(const int* ids_a, const unsigned char* lab_a, long long n_a, const int* ids_b,
                   const unsigned char* lab_b, long long n_b, long long V, unsigned char* hit_a,
                   unsigned char* hit_b, void* stream);

/* ---- multi-planar slicer (PMU/utils/mri_dataset.py:11-143) --------------------------------
 * A scan vol [d0][d1][d2] (f64) is re-laid out per view into a padded p0 x p1 x p2 frame
 * (pad_dimensions :85-98 = zeros at the end of the argmin axis) so each slice is contiguous:
 *   view 0: out[i][j][k] (slice = image[i,:,:]),  view 1: out[j][i][k] (image[:,j,:]),
 *   view 2: out[k][i][j] (image[:,:,k])            (sample_slice :70-82). */
int pmu_slice_view_layout(const double* vol, int d0, int d1, int d2, int p0, int p1, int p2, int view,
                          double* out, void* stream);
/* out[s] = max over the px elements of slice s (preprocess' max :109-110, index-map filter :45-46). */
int pmu_slice_max(const double* slices, int nslices, long long px, double* out, void* stream);
/* Batch assembly from a device slice table: addr[g] = device address of f64 slice g (px elements),
 * maxv[g] its max.  out[b][:] = float(slice[ids[b]] / maxv[ids[b]]) when normalize and the max is
 * non-zero, else float(value) (preprocess :101-112 then .float() :142).  ids: device [B]. */
int pmu_gather_slices(const long long* addr, const double* maxv, const int* ids, int B, long long px,
                      int normalize, float* out, void* stream);

/* ---- 3-view volume fusion (PMU/eval.py:157-203) --------------------------------------------
 * v0 [D0][C][D1][D2], v1 [D1][C][D0][D2], v2 [D2][C][D0][D1]: the per-view stacks of slice
 * predictions (probabilities; logits=1 applies softmax over C first).  In the view-0 frame:
 * avg = (p0 + p1 + p2) / 3 (optional output, [D0][C][D1][D2]), label = first argmax of avg
 * (optional, int32 [D0][D1][D2]), and counts[4][C][3] = exact (intersection, |pred|, |truth|) of the
 * one-hot argmax of view 0, view 1, view 2 and avg vs truth [D0][D1][D2] == c.  C <= 8. */
int pmu_fuse3view(const float* v0, const float* v1, const float* v2, const float* truth, int D0, int D1,
                  int D2, int C, int logits, float* avg, int* label, double* counts, void* stream);

/* ---- oblique view planes (extends PMU/utils/mri_dataset.py:60-66 and PMU/eval.py:157-203) ---
 * The reference defines only the standard axes (initialize_views leaves use_standard_axis=False
 * undefined); these entries slice and fuse along any unit vector.  A frame is nine doubles
 * n[3] u[3] v[3] (orthonormal; n the slicing direction).  vol is the padded volume [p0][p1][p2] (f64:
 * pmu_slice_view_layout's view 0) with centre c = (p - 1) / 2.  A view is a P x P x P grid of spacing h
 * voxels about c: slice s, pixel (a, b) sits at x = c + ((ds n + da u) + db v), d. = h (. - (P-1)/2),
 * evaluated in fp64 in this order without contraction.  Image samples are trilinear in fp64
 * (a + f (b - a) along axis 2, 1, 0; voxels outside read as 0), mask samples (nearest != 0) the voxel
 * floor(x + 0.5) or 0 outside. */
/* out[s] = max over the P*P samples of slice s, s < P, sampled on the fly (extends mri_dataset.py:60-66:
 * preprocess' max and the index-map filter for a view along frame). */
int pmu_oblique_slice_max(const double* vol, int p0, int p1, int p2, const double* frame, int P, double h,
                          int nearest, double* out, void* stream);
/* Batch assembly (extends mri_dataset.py:60-66): item ids[b] = r * P + s is slice s of table row r
 * (one row per scan and view: vaddr[r] the volume's device address, dims[r][3] its padded dims,
 * frames[r][9] the view's frame), r < nrows.  out[b][a][b'] = float(sample / maxv[ids[b]]) when maxv is
 * given and that max is non-zero, else float(sample).  ids: device [B]; out: [B][P][P]. */
int pmu_oblique_gather(const long long* vaddr, const int* dims, const double* frames, const double* maxv,
                       const int* ids, int B, int nrows, int P, double h, int nearest, float* out, void* stream);
/* Fusion of V <= 8 oblique views (extends eval.py:157-203).  stacks [V][P][C][P][P]: per-view stacks of
 * slice probabilities, C <= 8; frames [V][9]; truth [p0][p1][p2] labels.  Voxel x maps to view
 * coordinates g. = ((d0 f0 + d1 f1) + d2 f2) / h + (P-1)/2, d = x - c, f = n, u, v (fp64, no
 * contraction); a view covers the voxel iff 0 <= g <= P-1 on all three; its probability there is the
 * fp32 trilinear a + w (b - a) along the stack's W, H, then slice axis over the cell at floor(g)
 * (upper neighbour clamped to P-1), w = (float)(g - floor(g)).  avg (optional, [p0][C][p1][p2]) = the
 * fp32 sum over the covering views in view order / their number, zeros where none covers; label
 * (optional, int32) its first maximum; cover (optional, int32) that number; counts[(V+1)][C][3] = exact
 * (intersection, |pred|, |truth|) of each view's own first-maximum label (0 where it does not cover)
 * and of label, vs truth == c. */
int pmu_fuse_oblique(const float* stacks, const double* frames, int V, int C, int P, double h, const float* truth,
                     int p0, int p1, int p2, float* avg, int* label, int* cover, double* counts, void* stream);

/* ---- learned multi-planar fusion (extends PMU/eval.py:157-203; DESIGN.md "Learned fusion") ----
 * The plain mean of the views is replaced by a fusion model with one weight per view and class and one
 * bias per class: z_c(x) = b_c + sum_v W[v][c] p_{v,c}(x), fused = softmax(z), label = first maximum of z.
 * params: HOST array of V C + C doubles, W[v][c] then b[c]; cw: HOST array of C per-class loss weights
 * (>= 0) or null (ones).  Both are read before the entry returns and travel in the kernel arguments.
 * 2 <= C <= 8.  Per voxel, in fp64 and in this order, without contraction: z_c = b_c; z_c = z_c + W[v][c]
 * (double)p_{v,c} for v in view order; m = max_c z_c; s = sum_c exp(z_c - m) in class order; q_c =
 * exp(z_c - m) / s; with t = (int)truth a voxel with t outside [0, C) has fit weight 0, else w = cw[t];
 * l = w ((log s + m) - z_t); dz_c = w (q_c - [c == t]).
 * Outputs, each optional (null: not computed): prob = (float)q in the layout of the plain-mean avg; label
 * (int32); counts[(V+1)][C][3] = the plain-mean entry's exact counters, rows 0..V-1 unchanged (each view's
 * own first-maximum label), row V the learned fusion's label; sums[K], K = 2 + C + V C doubles, un-normalised:
 * [sum w, sum l, sum dz_c (C), sum dz_c p_{v,c} (V C, view-major)] — the fit's loss is sums[1] / sums[0] and its
 * gradient in (b, W) is sums[2:] / sums[0].  The sums are reproducible bit for bit (no floating-point
 * atomics: fp64 per thread, a fixed-order wave and block tree, one row per block in ws, a single block that
 * totals the rows in order); accumulate != 0 adds the call's total to sums instead of storing it, so several
 * scans sum on the device in call order.  sums needs ws, 8-byte aligned, of at least the *_ws query's bytes. */
/* The three standard views: the stacks, the view-0 frame and the logits flag (the same fp32 softmax first)
 * of pmu_fuse3view; V = 3. */
size_t pmu_fusion3_ws(int D0, int D1, int D2, int C);
int pmu_fusion3_eval(const float* v0, const float* v1, const float* v2, const float* truth, int D0, int D1, int D2,
                     int C, int logits, const double* params, const double* cw, float* prob, int* label,
                     double* counts, double* sums, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* 1 <= V <= 8 oblique views: the geometry, the coverage rule and the fp32 trilinear resampling of
 * pmu_fuse_oblique (a view's resampled probability is the same bits).  A view that does not cover a voxel
 * contributes nothing to z (nor to the W gradient there); a voxel no view covers gets probability 0 and
 * label 0 and is left out of the sums, and of nothing else.  cover (optional, int32) as pmu_fuse_oblique's. */
size_t pmu_fusion_oblique_ws(int V, int C, int p0, int p1, int p2);
int pmu_fusion_oblique_eval(const float* stacks, const double* frames, int V, int C, int P, double h,
                            const float* truth, int p0, int p1, int p2, const double* params, const double* cw,
                            float* prob, int* label, int* cover, double* counts, double* sums, int accumulate,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- on-the-fly slice augmentation (extension; the reference trains on un-augmented slices) ---
 * The warped batch gather: image and mask of B items in one launch, sampled from the resident padded
 * volumes through a per-item in-plane affine map plus a cubic B-spline elastic displacement (DESIGN.md,
 * "Augmentation").  The tables are pmu_oblique_gather's (row r < nrows: vaddr_img[r] / vaddr_mask[r] the
 * volumes, dims[r][3], frames[r][9]).  Item b: item[b] = (row, index into maxv), par[b] = [ds, m00, m01,
 * m10, m11, ta, tb, gain, bias], ctrl[b][2][G][G] plane displacements in voxels (G = 0 and ctrl null: no
 * elastic part; else 4 <= G <= 16).  Output pixel (a, b) of H x W at spacing h, all fp64, no contraction:
 *   pa = h (a - (H-1)/2), pb = h (b - (W-1)/2);
 *   d_k = sum_i wa_i (((wb_0 c_i0 + wb_1 c_i1) + wb_2 c_i2) + wb_3 c_i3), c_ij = ctrl[b][k][ia+i][ib+j], with
 *     ua = a ((G-3) / (H-1)), ia = min(floor(ua), G-4), t = ua - ia and the uniform cubic B-spline weights
 *     w0 = (1-t)^3 / 6, w1 = ((3 t^3 - 6 t^2) + 4) / 6, w2 = (((-3 t^3 + 3 t^2) + 3 t) + 1) / 6, w3 = t^3 / 6
 *     (the same along b with W);
 *   qa = (m00 (pa + d_0) + m01 (pb + d_1)) + ta, qb = (m10 (pa + d_0) + m11 (pb + d_1)) + tb;
 *   x = c + ((ds n + qa u) + qb v);
 *   img_out[b][a][b'] = float(y gain + bias), y = trilinear(x) / maxv[index] when maxv is given and that max
 *     is non-zero, else trilinear(x);  mask_out[b][a][b'] = float(nearest(x)).
 * Either output may be null (not both); maxv may be null.  With M = I, t = 0, G = 0, gain 1, bias 0 the
 * outputs equal pmu_oblique_gather's (H = W = P, ds = h (s - (P-1)/2)) bit for bit. */
int pmu_warp_gather(const long long* vaddr_img, const long long* vaddr_mask, const int* dims, const double* frames,
                    int nrows, const int* item, const double* maxv, const double* par, const double* ctrl, int G,
                    int B, int H, int W, double h, float* img_out, float* mask_out, void* stream);

/* ---- probabilistic path: latent head of AxisAlignedConvGaussian ---------------------------
 * probabilistic_unet.py:95-108: encoding = mean_{h,w} relu(bn(z_last)); mu_log_sigma = conv1x1(encoding). */
/* out[N][C] = (1/(H*W)) sum_{h,w} max(0, z*scale+shift), z NHWC, coef = [scale|shift]. */
int pmu_spatial_mean(const float* z, const float* coef, int N, int H, int W, int C, float* out,
                     void* stream);
/* da[N][H][W][C] = dmean[N][C] / (H*W). */
int pmu_spatial_mean_bwd(const float* dmean, int N, int H, int W, int C, float* da, void* stream);
/* The same fused with the BN+ReLU backward partial sums of the averaged layer (:39 mean over the
 * encoder's last activation): part as pmu_avgpool2_bwd_bnr.  C % 4 == 0. */
int pmu_spatial_mean_bwd_bnr(const float* dmean, const float* z, const float* coef, const float* mean,
                             const float* invstd, int N, int H, int W, int C, float* da, float* part, void* stream);
/* y[N][M] = x[N][K] . w[M][K]^T + b  (a 1x1 conv on a 1x1 map, probabilistic_unet.py:72,101). */
int pmu_linear_fwd(const float* x, const float* w, const float* b, int N, int K, int M, float* y,
                   void* stream);
/* dx = dy.w (dx may be NULL), dw = dy^T.x, db = sum_n dy (db may be NULL); M <= 256. */
int pmu_linear_bwd(const float* x, const float* w, const float* dy, int N, int K, int M, float* dx,
                   float* dw, float* db, void* stream);

/* ---- probabilistic path: Fcomb (probabilistic_unet.py:116-181) ----------------------------
 * logits = W_last . relu(W_NH ... relu(W_1 . cat(f, tile(z)) + b_1) ...) + b_last per pixel,
 * NH = no_convs_fcomb - 1 hidden 1x1 convs (1..3), F = feature width (<= 64), L = latent dim,
 * K = classes (<= 32).  w[l], b[l]: PyTorch layouts (w[0] = W_1 [F][F+L], w[l>0] = [F][F]),
 * wl = W_last [K][F].  The tiled z is never built: zb = W_1z . z + b_1 is a per-(sample,image)
 * bias from pmu_fcomb_zbias. */
/* zb[SN][F] = w1[:, F:F+L] . z[SN][L] + b1. */
int pmu_fcomb_zbias(const float* z, const float* w1, const float* b1, int SN, int F, int L,
                    float* zb, void* stream);
/* feat NHWC [N][H][W][F]; zb [S][N][F]; y NCHW [S][N][K][H][W] (S samples in one pass). */
int pmu_fcomb_fwd(const float* feat, const float* zb, const float* const* w, const float* const* b,
                  const float* wl, const float* bl, int F, int L, int K, int NH, int S, int N, int H,
                  int W, float* y, void* stream);
/* Sample statistics without the S logit tensors: the inputs and ranges of pmu_fcomb_fwd (F <= 64, NH 1..3,
 * K 1..32, L >= 0, S >= 1), every output element overwritten.  With p_s = softmax(y_s) over the K classes
 * (K == 1: p_s = sigmoid(y_s), entropies of the Bernoulli [1 - p, p]; mean keeps one channel):
 *   mean    [N][K][H][W] f32   (1/S) sum_s p_s
 *   entropy [N][H][W]    f32   H(mean) = -sum_k mean_k ln mean_k (nats, 0 ln 0 = 0)
 *   mi      [N][H][W]    f32   max(0, H(mean) - (1/S) sum_s H(p_s))
 *   label   [N][H][W]    i32   first argmax of mean (K == 1: mean > 0.5); may be NULL
 *   labels  [S][N][H][W] u8    first argmax of y_s (K == 1: y_s > 0); may be NULL */
int pmu_fcomb_stats(const float* feat, const float* zb, const float* const* w, const float* const* b,
                    const float* wl, const float* bl, int F, int L, int K, int NH, int S, int N, int H,
                    int W, float* mean, float* entropy, float* mi, int* label, unsigned char* labels,
                    void* stream);
size_t pmu_fcomb_bwd_ws(int N, int H, int W);
/* One sample: dl = dL/dlogits NCHW [N][K][H][W] -> dfeat NHWC, dz [N][L] (may be NULL),
 * dw[l], db[l] (PyTorch layouts, overwritten), dwl, dbl.  z [N][L] and zb [N][F] as in forward. */
int pmu_fcomb_bwd(const float* feat, const float* z, const float* zb, const float* dl,
                  const float* const* w, const float* const* b, const float* wl, const float* bl,
                  int F, int L, int K, int NH, int N, int H, int W, float* dfeat, float* dz,
                  float* const* dw, float* const* db, float* dwl, float* dbl, float* ws,
                  size_t ws_bytes, void* stream);

/* ---- diagnostics: resident blocks per CU of the main GEMM kernels (hipOccupancy API) ---- */
int pmu_occupancy_conv3x3_raw(int* blocks_per_cu);
int pmu_occupancy_wgrad3x3_bf16(int* blocks_per_cu);

/* ---- batched weight packing ------------------------------------------------------------------
 * One launch re-packs the weights of many layers into one layout after an optimizer step
 * (pmu_hip.optim.FusedSGD -> pmu_hip.engine.repack): jobs[] in DEVICE memory, job j = one tensor w
 * [Cout][Cin][3][3] (ConvTranspose2d: [Cin][Cout][2][2]) packed into dst as the single-tensor pack
 * function of that layout would, using workgroups [block0, block0 + nblocks) of a grid of `blocks`
 * (nblocks from the matching *_blocks query).  dgrad is uniform over the jobs of one call. */
typedef struct {
  const float* w;
  void* dst;
  int Cout, Cin, block0, nblocks;
} pmu_pack_job;
int pmu_conv3x3_pack_wino2h_blocks(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_wino2h_multi(const pmu_pack_job* jobs, int njobs, int blocks, int dgrad, void* stream);
int pmu_conv3x3_pack_wino4_blocks(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_wino4_multi(const pmu_pack_job* jobs, int njobs, int blocks, int dgrad, void* stream);
int pmu_convT2x2_pack_blocks(int Cin, int Cout, int dgrad);
int pmu_convT2x2_pack_multi(const pmu_pack_job* jobs, int njobs, int blocks, int dgrad, void* stream);
int pmu_conv3x3_pack_dma_blocks(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack_dma_multi(const pmu_pack_job* jobs, int njobs, int blocks, int dgrad, void* stream);
int pmu_convT2x2_pack_dma_blocks(int Cin, int Cout, int dgrad);
int pmu_convT2x2_pack_dma_multi(const pmu_pack_job* jobs, int njobs, int blocks, int dgrad, void* stream);

/* ---- build identity and the bounds-checked debug build ------------------------------------ */
/* Bit 0: experiments build (make EXPERIMENTS=1: kernel-variant A/B switches honoured); bit 1:
 * bounds-checked debug build (make DEBUG=1 -> libpmunet_hip_debug.so, PMU_DCHECK in the kernels). */
int pmu_build_flags(void);
/* Debug build: synchronises the device and returns the first recorded index-bound violation,
 * out[0..4] = {code (PMU_DBG_* in csrc/pmu_common.h; 0 = none), source line, workgroup, set,
 * translation unit}; *tu_name (may be NULL) receives the source file.  Release build: out all 0.
 * pmu_debug_reset clears the records. */
int pmu_debug_read(int* out, const char** tu_name);
int pmu_debug_reset(void);

#ifdef __cplusplus
}
#endif
#endif
