/* libpmunet_hip EXPERIMENTS build only (csrc: make EXPERIMENTS=1 -> pmu_hip/libpmunet_hip_exp.so).
 *
 * Kernels that were built, tested against fp64 / the oracle and measured, but that the engine's
 * default dispatch does not reach: an independent implementation the tests compare against (the
 * direct-sum fp32 conv) and kernels that break the parity contract, an accuracy question still open
 * (F(4x4) forward, bf16-stored z).  They stay buildable (PMU_LIB=exp, tools/kbench*.py, the engine's
 * PMU_FP32_CONV / PMU_WINO4 / PMU_BF16_Z switches, which the shipped library ignores) and their tests
 * run against the experiments library (tests/conftest.py exp_lib).  Kernels kept only for a timing
 * A/B that has been settled were removed ("Removed A/B code").  Same types and conventions
 * as include/pmunet_hip.h. */
#ifndef PMUNET_HIP_EXPERIMENTS_H
#define PMUNET_HIP_EXPERIMENTS_H

#include "pmunet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- direct-sum fp32 3x3 convolution (implicit GEMM, fused staging): PMU_FP32_CONV=direct */
/* z[N][H][W][Cout] = conv3x3(frame, w) + bias.  If part != NULL, per-tile BN partial
 * sums (sum z, sum z^2) are written to part[tile][2][Cout]; pmu_conv3x3_tiles() gives
 * the tile count.  tee (nullable): receives the operand the kernel multiplied (the frame after
 * BN+ReLU / pooling / concatenation), [N][H][W][Cin] fp32 — a RAW source for pmu_conv3x3_wgrad. */
int pmu_conv3x3_fwd(const pmu_frame* in, const float* w, const float* wp, const float* bias,
                    int Cout, float* z, float* part, float* tee, void* stream);
/* Optional pre-packed weights (wp != NULL replaces w): the per-block/chunk B tiles laid out
 * contiguously in LDS order, so staging is a straight copy.  dgrad=1 packs the flipped,
 * transposed operand of pmu_conv3x3_dgrad. */
size_t pmu_conv3x3_packed_size(int Cout, int Cin, int dgrad);
int pmu_conv3x3_pack(const float* w, int Cout, int Cin, int dgrad, float* wp, void* stream);
/* dx = dL/d(frame) for frame channels [0,Csplit) -> dx0 (NHWC, Csplit ch) and
 * [Csplit,Cin) -> dx1 (NHWC, Cin-Csplit ch).  dz is a frame whose single source is
 * normally PMU_SRC_BNBWD. */
int pmu_conv3x3_dgrad(const pmu_frame* dz, const float* w, const float* wp, int Cin, int Csplit,
                      float* dx0, float* dx1, float* tee, void* stream);  /* tee: dz after BN backward, [N][H][W][Cout] */

/* ---- F(4x4,3x3) forward: breaks the model-level 1e-3 / Dice contract through the BatchNorm statistics
 * (DESIGN.md §3a); PMU_WINO4=1 */
int pmu_conv3x3_fwd_wino4(const float* xt, int Cin, int N, int H, int W, const float* wp, const float* bias,
                          int Cout, float* z, float* part, void* stream);

/* ---- bf16-stored z: breaks the c5 eval Dice contract and is not faster; PMU_BF16_Z=1 */
/* bf16 storage of z (config c5: torch.autocast keeps a conv's output in bf16, unet_parts.py:15,18 under
 * autocast), centred: the forward stores bf16(z - zoff[c]) (RNE; zoff = the BN running mean, null: 0)
 * with the BN partial sums of stored + zoff; every consumer then applies the centred coefficients of
 * pmu_bn_center.  The input gradient's BN-backward partials read such a z. */
int pmu_conv3x3_fwd_dma_zb(const unsigned short* xt, int Cp, int N, int H, int W, const unsigned short* wp,
                           const float* bias, int Cout, unsigned short* z, const float* zoff, float* part,
                           void* stream);
/* coef_out = [scale | shift + off*scale], mean_out = mean - off (in place allowed; mean may be NULL) */
int pmu_bn_center(const float* coef, const float* mean, const float* off, int C, float* coef_out,
                  float* mean_out, void* stream);
int pmu_conv3x3_dgrad_dma_bnr_zb(const unsigned short* dzt, int Cp, int N, int H, int W, const unsigned short* wp,
                                 int Cin, float* dx, const unsigned short* z, const float* coef, const float* mean,
                                 const float* invstd, float* part, void* stream);

/* the same over a bf16-stored z (C % 4 == 0) */
int pmu_bn_bwd_reduce_zb(const float* da, const unsigned short* z, const float* coef, const float* mean,
                         const float* invstd, int P, int C, float* part, void* stream);

/* the same over a bf16-stored z (coef required, C % 4 == 0) */
int pmu_maxpool2_bwd_zb(const float* dpool, const unsigned short* z, const float* coef, int N, int H, int W,
                        int C, float* dx, int accumulate, void* stream);

/* ---- diagnostics of the direct-sum kernel */
int pmu_occupancy_conv3x3_pipe(int* blocks_per_cu);

#ifdef __cplusplus
}
#endif

#endif  /* PMUNET_HIP_EXPERIMENTS_H */
