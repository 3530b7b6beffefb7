/*
 * oracle/svt_oracle.h - TEST INFRASTRUCTURE ONLY.
 *
 * Plain-C restatement of the SVT-HEVC block-analysis hot path, used as the
 * bit-exact checker for the HIP path (tests/, __graft_entry__.smoke(),
 * bench.py's cpu_baseline leg).  Nothing in the product (svt-hevc_amd/) may
 * include, link or call this.  Pinning: every function here is checked against
 * the reference itself, compiled into oracle/_ref/libsvtref.so from
 * /root/reference (tests/test_oracle_vs_ref.py) and against golden fixtures
 * produced by that build (tests/golden/, tests/golden/make_me_golden.py).
 *
 * Each function cites the reference file:line it restates
 * (paths relative to /root/reference/Source/Lib).
 */
#ifndef SVT_ORACLE_H
#define SVT_ORACLE_H

#include <stdint.h>
#include <stddef.h>
#include "../include/svt_hevc_amd.h"

#ifdef __cplusplus
extern "C" {

/* ---- SAO parameter decision of one LCU (svt_oracle_saodec.c) ---- */
void svt_oracle_sao_decide_lcu(const SvtAmdSaoDecisionParams *P, const SvtAmdSaoStats *const stats[3], const SvtAmdSaoLcuParams *left,
                               const SvtAmdSaoLcuParams *up, SvtAmdSaoLcuParams *out, int64_t costs[2]);
void svt_oracle_sao_decide_picture(const SvtAmdSaoDecisionParams *P, const SvtAmdSaoStats *sy, const SvtAmdSaoStats *scb,
                                   const SvtAmdSaoStats *scr, uint32_t cols, uint32_t rows, const uint8_t *enable,
                                   SvtAmdSaoLcuParams *params, int64_t *costs);

#endif

/* ---- leaf kernels (same signatures as the reference C_DEFAULT symbols) ---- */
void svt_oracle_fast_loop_distortion(const SvtAmdFastLoopCand *K, const uint8_t *srcY, uint32_t srcStrideY, const uint8_t *srcCb,
                                     const uint8_t *srcCr, uint32_t srcStrideC, const uint8_t *predY, uint32_t predStrideY,
                                     const uint8_t *predCb, const uint8_t *predCr, uint32_t predStrideC, SvtAmdFastLoopDist *out);
uint32_t svt_oracle_NxMSadKernel(const uint8_t *src, uint32_t srcStride, const uint8_t *ref,
                                 uint32_t refStride, uint32_t height, uint32_t width);
void svt_oracle_SadLoopKernel(const uint8_t *src, uint32_t srcStride, const uint8_t *ref,
                              uint32_t refStride, uint32_t height, uint32_t width,
                              uint64_t *bestSad, int16_t *xSearchCenter, int16_t *ySearchCenter,
                              uint32_t srcStrideRaw, int16_t searchAreaWidth,
                              int16_t searchAreaHeight);
uint32_t svt_oracle_NxMSadAveragingKernel(const uint8_t *src, uint32_t srcStride,
                                          const uint8_t *ref1, uint32_t ref1Stride,
                                          const uint8_t *ref2, uint32_t ref2Stride,
                                          uint32_t height, uint32_t width);
void svt_oracle_GetEightHorizontalSearchPointResults_8x8_16x16_PU(
    const uint8_t *src, uint32_t srcStride, const uint8_t *ref, uint32_t refStride,
    uint32_t *pBestSad8x8, uint32_t *pBestMV8x8, uint32_t *pBestSad16x16,
    uint32_t *pBestMV16x16, uint32_t mv, uint16_t *pSad16x16);
void svt_oracle_GetEightHorizontalSearchPointResults_32x32_64x64(
    const uint16_t *pSad16x16, uint32_t *pBestSad32x32, uint32_t *pBestSad64x64,
    uint32_t *pBestMV32x32, uint32_t *pBestMV64x64, uint32_t mv);
void svt_oracle_SadCalculation_8x8_16x16(const uint8_t *src, uint32_t srcStride,
                                         const uint8_t *ref, uint32_t refStride,
                                         uint32_t *pBestSad8x8, uint32_t *pBestSad16x16,
                                         uint32_t *pBestMV8x8, uint32_t *pBestMV16x16,
                                         uint32_t mv, uint32_t *pSad16x16);
void svt_oracle_SadCalculation_32x32_64x64(const uint32_t *pSad16x16, uint32_t *pBestSad32x32,
                                           uint32_t *pBestSad64x64, uint32_t *pBestMV32x32,
                                           uint32_t *pBestMV64x64, uint32_t mv);
void svt_oracle_AvcStyleLumaInterpolationFilterHorizontal(
    const uint8_t *refPic, uint32_t srcStride, uint8_t *dst, uint32_t dstStride,
    uint32_t puWidth, uint32_t puHeight, uint8_t *tempBuf, uint32_t fracPos);
void svt_oracle_AvcStyleLumaInterpolationFilterVertical(
    const uint8_t *refPic, uint32_t srcStride, uint8_t *dst, uint32_t dstStride,
    uint32_t puWidth, uint32_t puHeight, uint8_t *tempBuf, uint32_t fracPos);
void svt_oracle_PictureAverageKernel(const uint8_t *src0, uint32_t src0Stride,
                                     const uint8_t *src1, uint32_t src1Stride, uint8_t *dst,
                                     uint32_t dstStride, uint32_t areaWidth, uint32_t areaHeight);
uint64_t svt_oracle_SpatialFullDistortionKernel(const uint8_t *input, uint32_t inputStride,
                                                const uint8_t *recon, uint32_t reconStride,
                                                uint32_t areaWidth, uint32_t areaHeight);
void svt_oracle_Decimation2D(const uint8_t *inputSamples, uint32_t inputStride,
                             uint32_t inputAreaWidth, uint32_t inputAreaHeight,
                             uint8_t *decimSamples, uint32_t decimStride, uint32_t decimStep);

/* ---- residual / transform / quantisation / distortion / SATD leaves ------- */
/* kind: 0 DCT, 1 low-precision "Estimate" DCT (32/16), 2 DST (4x4); inner may be NULL */
void svt_oracle_FwdTransform(int kind, int size, const int16_t *residual, uint32_t srcStride, int16_t *coeff,
                             uint32_t dstStride, int16_t *inner, uint32_t bitIncrement);
void svt_oracle_InvTransform(int kind, int size, const int16_t *coeff, uint32_t srcStride, int16_t *residual,
                             uint32_t dstStride, int16_t *inner, uint32_t bitIncrement);
void svt_oracle_QuantizeInvQuantize(const int16_t *coeff, uint32_t coeffStride, int16_t *quantCoeff,
                                    int16_t *reconCoeff, uint32_t qFunc, uint32_t q_offset, int32_t shiftedQBits,
                                    int32_t shiftedFFunc, int32_t iq_offset, int32_t shiftNum, uint32_t areaSize,
                                    uint32_t *nonzerocoeff);
void svt_oracle_UpdateQiQCoef(int16_t *quantCoeff, int16_t *reconCoeff, uint32_t coeffStride, int32_t shiftedFFunc,
                              int32_t iq_offset, int32_t shiftNum, uint32_t areaSize, uint32_t *nonzerocoeff,
                              uint32_t componentType, uint32_t sliceType, uint32_t temporalLayer,
                              uint32_t enableCbflag, uint8_t enableContouringQCUpdateFlag);
/* the encode pass's quantiser without RDOQ / masking (composite of the two above + shape / dead-zone / clean-up) */
void svt_oracle_unified_quantize(const SvtAmdQuantUnit *unit, const int16_t *coeff, uint32_t stride, int16_t *quant, int16_t *recon,
                                 uint32_t *nz);
void svt_oracle_ResidualKernel(const uint8_t *input, uint32_t inputStride, const uint8_t *pred, uint32_t predStride,
                               int16_t *residual, uint32_t residualStride, uint32_t w, uint32_t h);
void svt_oracle_PictureAdditionKernel(const uint8_t *pred, uint32_t predStride, const int16_t *residual,
                                      uint32_t residualStride, uint8_t *recon, uint32_t reconStride, uint32_t w,
                                      uint32_t h);
void svt_oracle_ZeroOutCoeffKernel(int16_t *coeff, uint32_t stride, uint32_t origin, uint32_t w, uint32_t h);
/* mode: 0 FullDistortionKernel_32bit, 1 ...CbfZero_32bit, 2 ...Intra_32bit */
void svt_oracle_FullDistortionKernel_32bit(const int16_t *coeff, uint32_t coeffStride, const int16_t *recon,
                                           uint32_t reconStride, uint64_t result[2], uint32_t w, uint32_t h, int mode);
uint64_t svt_oracle_Compute8x8Satd(const int16_t *diff);
uint64_t svt_oracle_Compute4x4Satd(const int16_t *diff);
uint64_t svt_oracle_Compute8x8Satd_U8(const uint8_t *src, uint64_t *dcValue, uint32_t srcStride);
uint64_t svt_oracle_Compute4x4Satd_U8(const uint8_t *src, uint64_t *dcValue, uint32_t srcStride);

/* ---- intra prediction leaves (C_DEFAULT/EbIntraPrediction_C.c) ------------ */
enum {
    SVT_ORACLE_INTRA_VERTICAL_LUMA = 0, SVT_ORACLE_INTRA_VERTICAL_CHROMA, SVT_ORACLE_INTRA_HORIZONTAL_LUMA,
    SVT_ORACLE_INTRA_HORIZONTAL_CHROMA, SVT_ORACLE_INTRA_DC_LUMA, SVT_ORACLE_INTRA_DC_CHROMA, SVT_ORACLE_INTRA_PLANAR,
    SVT_ORACLE_INTRA_ANGULAR_34, SVT_ORACLE_INTRA_ANGULAR_18, SVT_ORACLE_INTRA_ANGULAR_2,
    SVT_ORACLE_INTRA_ANGULAR_VERTICAL, SVT_ORACLE_INTRA_ANGULAR_HORIZONTAL
};
/* bps: 1 (8-bit kernels) or 2 (16-bit kernels); ref is refSamples, or refSampMain for the two generic
 * angular kernels; stride in samples */
void svt_oracle_IntraPred(int mode, int bps, uint32_t size, const void *ref, void *pred, uint32_t stride, int skip,
                          int32_t intraPredAngle);
/* encode-pass intra prediction of one prediction unit from neighbour-array slices (composite, see svt_oracle_intra.c) */
void svt_oracle_intra_pu(int bps, const SvtAmdIntraPuJob *job, void *pred_y, uint32_t strideY, void *pred_cb, void *pred_cr,
                         uint32_t strideC);

/* ---- in-loop filters and bit-depth packing leaves (bps: 1 = 8-bit kernels, 2 = *16bit kernels) ---- */
void svt_oracle_Luma4SampleEdgeDLFCore(int bps, void *edge, uint32_t stride, int isVerticalEdge, int32_t tc, int32_t beta);
void svt_oracle_Chroma2SampleEdgeDLFCore(int bps, void *cb, void *cr, uint32_t stride, int isVerticalEdge,
                                         uint8_t cbTc, uint8_t crTc);
/* whole-picture deblocking = the result of the three per-LCU drivers over all LCUs (4:2:0; tight or strided planes) */
void svt_oracle_dlf_picture(int bps, void *y, uint32_t strideY, void *cb, void *cr, uint32_t strideC, uint32_t width,
                            uint32_t height, const uint8_t *bs_v, const uint8_t *bs_h, const uint8_t *qp, uint32_t qpStride,
                            int tcOffset, int betaOffset, int cbQpOffset, int crQpOffset);
/* picture-level boundary-strength derivation from coding-unit / cbf maps (see svt_oracle_loopfilter.c) */
typedef struct SvtOracleCuMapEntry { uint8_t mode, dir, size_log2, pad; int16_t mv[2][2]; } SvtOracleCuMapEntry;
void svt_oracle_bs_picture(const SvtOracleCuMapEntry *map, const uint8_t *cbf, uint32_t width, uint32_t height, int sliceType,
                           const uint64_t refPoc[2], const uint8_t *lcuEdge, uint8_t *bs_v, uint8_t *bs_h);
/* whole-picture SAO application (out of place); one parameter record per LCU, same field order as SaoParameters_t after
 * the two merge flags (Codec/EbCodingUnit.h:137-146) plus the tile-edge flags ApplySaoOffsetsLcu reads */
typedef struct SvtOracleSaoLcu {
    uint8_t merge_left, merge_up, edge_flags /* 1 left, 2 right, 4 top, 8 bottom tile edge */, pad;
    uint32_t type[2];
    int32_t offset[3][4];
    uint32_t band[3];
} SvtOracleSaoLcu;
void svt_oracle_sao_apply_picture(int bps, const void *const src[3], void *const dst[3], uint32_t strideY, uint32_t strideC,
                                  uint32_t width, uint32_t height, const SvtOracleSaoLcu *lcus, int lumaOn, int chromaOn);
void svt_oracle_GatherSaoStatistics(int bps, int only_eo_90_45_135, const void *input, uint32_t inputStride,
                                    const void *recon, uint32_t reconStride, uint32_t lcuWidth, uint32_t lcuHeight,
                                    int32_t *boDiff, uint16_t *boCount, int32_t eoDiff[4][5], uint16_t eoCount[4][5]);
void svt_oracle_SAOApplyBO(int bps, void *recon, uint32_t stride, uint32_t bandPosition, const int8_t *offset,
                           uint32_t lcuHeight, uint32_t lcuWidth);
/* eoType 0: 0 deg (left only), 1: 90 (upper only), 2: 135, 3: 45 (left + upper, upper indexed -1..W) */
void svt_oracle_SAOApplyEO(int bps, int eoType, void *recon, uint32_t stride, const void *left, const void *upper,
                           const int8_t *offset, uint32_t lcuHeight, uint32_t lcuWidth);
void svt_oracle_msbPack2D(const uint8_t *in8, uint32_t in8Stride, const uint8_t *inn, uint16_t *out16, uint32_t innStride,
                          uint32_t outStride, uint32_t w, uint32_t h);
void svt_oracle_CompressedPackmsb(const uint8_t *in8, uint32_t in8Stride, const uint8_t *inn, uint16_t *out16,
                                  uint32_t innStride, uint32_t outStride, uint32_t w, uint32_t h);
void svt_oracle_CPack(const uint8_t *inn, uint32_t innStride, uint8_t *out, uint32_t outStride, uint32_t w, uint32_t h);
void svt_oracle_msbUnPack2D(const uint16_t *in16, uint32_t inStride, uint8_t *out8, uint8_t *outn, uint32_t out8Stride,
                            uint32_t outnStride, uint32_t w, uint32_t h);
void svt_oracle_UnpackAvg(const uint16_t *l0, uint32_t s0, const uint16_t *l1, uint32_t s1, uint8_t *dst,
                          uint32_t dstStride, uint32_t w, uint32_t h);

/* ---- picture-level ME (restates MotionEstimationKernel's LCU loop) -------- */

/* A padded 8-bit plane: sample (x,y), x in [-pad, width+pad), is
 * data[(y + pad) * stride + (x + pad)]. */
typedef struct SvtOraclePlane {
    uint8_t *data;
    uint32_t stride;
    uint32_t pad;
    uint32_t width, height;
} SvtOraclePlane;

/* Everything ME reads of one picture (EbPaReferenceObject_t + derived half-pel planes). */
typedef struct SvtOraclePicture {
    SvtOraclePlane full, quarter, sixteenth; /* inputPadded / quarterDecimated / sixteenthDecimated */
    SvtOraclePlane hp_b, hp_h, hp_j;         /* AVC-style half-pel planes, geometry of `full`       */
} SvtOraclePicture;

/* Build from a raw luma plane; returns NULL on allocation failure. */
SvtOraclePicture *svt_oracle_picture_create(const uint8_t *luma, uint32_t stride,
                                            uint32_t width, uint32_t height);
void svt_oracle_picture_destroy(SvtOraclePicture *pic);

/* ME of LCUs [lcu_begin, lcu_end) of one picture (raster LCU order);
 * out[] is indexed by absolute LCU index. */
int svt_oracle_me_picture(const SvtAmdMeParams *params, const SvtOraclePicture *cur,
                          const SvtOraclePicture *ref0, const SvtOraclePicture *ref1,
                          uint32_t lcu_begin, uint32_t lcu_end, SvtAmdMeLcuResult *out);

#ifdef __cplusplus
}

/* ---- SAO parameter decision of one LCU (svt_oracle_saodec.c) ---- */
void svt_oracle_sao_decide_lcu(const SvtAmdSaoDecisionParams *P, const SvtAmdSaoStats *const stats[3], const SvtAmdSaoLcuParams *left,
                               const SvtAmdSaoLcuParams *up, SvtAmdSaoLcuParams *out, int64_t costs[2]);
void svt_oracle_sao_decide_picture(const SvtAmdSaoDecisionParams *P, const SvtAmdSaoStats *sy, const SvtAmdSaoStats *scb,
                                   const SvtAmdSaoStats *scr, uint32_t cols, uint32_t rows, const uint8_t *enable,
                                   SvtAmdSaoLcuParams *params, int64_t *costs);

#endif
/* ---- open-loop intra search (svt_oracle_ois.c) ---- */
/* luma points at the picture origin (sample 0,0); reads never leave [0,W)x[0,H). me_sad: distortion[0] of the
 * LCU's 85 ME records (NULL for I pictures). */
void svt_oracle_ois_lcu(const SvtAmdOisParams *P, const uint8_t *luma, uint32_t stride, uint32_t lcu_x, uint32_t lcu_y,
                        const uint32_t *me_sad, SvtAmdOisLcuResult *out);

/* ---- HEVC motion-compensation interpolation (svt_oracle_mcp.c) ---- */
/* chroma: 0 luma (fx,fy quarter-pel 0..3), 1 chroma (eighth-pel 0..7); out_raw: int16 output with stride = w */
void svt_oracle_mcp(int bps, int chroma, int out_raw, uint32_t fx, uint32_t fy, const void *ref, uint32_t srcStride,
                    void *dst, uint32_t dstStride, uint32_t w, uint32_t h);
void svt_oracle_BiPredClipping(int bps, uint32_t w, uint32_t h, const int16_t *l0, const int16_t *l1, void *dst,
                               uint32_t dstStride, int32_t offset);
/* encode-pass inter prediction of one prediction unit, 8-bit 4:2:0 (composite of the two above) */
void svt_oracle_inter_pu(const SvtAmdInterPuJob *job, const SvtAmdRefPicture *ref0, const SvtAmdRefPicture *ref1, uint8_t *pred_y,
                         uint32_t strideY, uint8_t *pred_cb, uint8_t *pred_cr, uint32_t strideC);
void svt_oracle_inter_pu16bit(const SvtAmdInterPuJob *J, const SvtAmdRefPicture *ref0, const SvtAmdRefPicture *ref1, uint16_t *pred_y,
                              uint32_t strideY, uint16_t *pred_cb, uint16_t *pred_cr, uint32_t strideC);

/* ---- ComputeDecimatedZzSad (svt_oracle_zz.c); cur/prev point at sample (0,0) of the two source pictures ---- */
void svt_oracle_zz_sad_picture(const uint8_t *cur, const uint8_t *prev, uint32_t stride, uint32_t width, uint32_t height,
                               SvtAmdZzLcu *out);

/* ---- coefficient rate estimation (svt_oracle_rate.c) ---- */
uint64_t svt_oracle_coeff_bits_lossy(const SvtAmdCabacCost *C, uint32_t size, uint32_t type, uint32_t intraLumaMode,
                                     uint32_t intraChromaMode, const int16_t *coeff, uint32_t stride,
                                     uint32_t componentType, uint32_t numNonZeroCoeffs);
/* EstimateQuantizedCoefficients_generic_Update (Codec/EbEntropyCoding.c:2986): same pricing with real context states that
 * every context-coded bin updates.  ctx = CoeffCtxtMdl_t as SVT_ORACLE_COEFF_CTX_WORDS words (updated in place); returns
 * the amount added to *coeffBitsLong (15 fractional bits; the callers shift right by 15). */
#define SVT_ORACLE_COEFF_CTX_WORDS 136
uint64_t svt_oracle_coeff_bits_update(uint32_t *ctx, uint32_t size, uint32_t type, uint32_t intraLumaMode,
                                      uint32_t intraChromaMode, const int16_t *coeff, uint32_t stride,
                                      uint32_t componentType, uint32_t numNonZeroCoeffs);
extern const uint32_t svt_oracle_cabac_estimated_bits[128];
extern uint32_t svt_oracle_next_state_mps_lps[256];

/* ---- luma full loop of one candidate (svt_oracle_fullloop.c) ---- */
uint64_t svt_oracle_encode_plane(const uint8_t *src, uint8_t *rec, uint32_t stride, uint32_t width, uint32_t row0, uint32_t rows,
                                 uint32_t size, uint32_t qp, uint32_t slice_type);
void svt_oracle_pmcore_quantize(const SvtAmdCabacCost *cost, const SvtAmdPmQuantUnit *U, const int16_t *coeff, int16_t *quant,
                                int16_t *recon, uint32_t *nzOut);
void svt_oracle_product_full_loop_luma(const SvtAmdCabacCost *cost, const SvtAmdFullLoopIn *in, const int16_t *residual,
                                       int16_t *quant, int16_t *recon, SvtAmdFullLoopOut *out);
void svt_oracle_full_loop_chroma(const SvtAmdCabacCost *cost, const SvtAmdChromaLoopIn *in, const int16_t *const residual[2],
                                 int16_t *const quant[2], int16_t *const recon[2], SvtAmdChromaLoopOut *out);
/* reconstruction of one transform unit of one plane (inverse transform or DC shortcut + prediction, clipped) */
void svt_oracle_recon_tu(int bps, uint32_t size, int only_dc, int dst, const int16_t *coeff, const void *pred,
                         uint32_t predStride, void *recon, uint32_t reconStride);


/* ---- SAO parameter decision of one LCU (svt_oracle_saodec.c) ---- */
void svt_oracle_sao_decide_lcu(const SvtAmdSaoDecisionParams *P, const SvtAmdSaoStats *const stats[3], const SvtAmdSaoLcuParams *left,
                               const SvtAmdSaoLcuParams *up, SvtAmdSaoLcuParams *out, int64_t costs[2]);
void svt_oracle_sao_decide_picture(const SvtAmdSaoDecisionParams *P, const SvtAmdSaoStats *sy, const SvtAmdSaoStats *scb,
                                   const SvtAmdSaoStats *scr, uint32_t cols, uint32_t rows, const uint8_t *enable,
                                   SvtAmdSaoLcuParams *params, int64_t *costs);

/* coeffCabacUpdate forms of the two full loops: model = candBuffCoeffCtxModel, SVT_ORACLE_COEFF_CTX_WORDS words, in / out */
void svt_oracle_product_full_loop_luma_cabac(const SvtAmdCabacCost *cost, const SvtAmdFullLoopIn *in, const int16_t *residual,
                                             int16_t *quant, int16_t *recon, uint32_t *model, SvtAmdFullLoopOut *out);
void svt_oracle_full_loop_chroma_cabac(const SvtAmdCabacCost *cost, const SvtAmdChromaLoopIn *in, const int16_t *const residual[2],
                                       int16_t *const quant[2], int16_t *const recon[2], uint32_t *model, SvtAmdChromaLoopOut *out);

/* The mode decision of a whole picture (svt_oracle_md.c): ModeDecisionLcu of every LCU in raster order */
uint32_t svt_oracle_md_mv_bits(int dx, int dy); /* mvBitTable[dx][dy] in closed form (md_logic.h:md_mv_bits) */
int svt_oracle_md_picture(const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus, const SvtAmdCabacCost *cost, const uint8_t *src_y, uint32_t stride,
                          const SvtAmdOisLcuResult *ois, SvtAmdMdLcuOut *out, uint8_t *md_rec);
int svt_oracle_md_picture_inter(const SvtAmdMdPicture *P, const SvtAmdMdInter *X, const SvtAmdMdLcu *lcus, const SvtAmdCabacCost *cost,
                                const uint8_t *src_y, uint32_t stride, const uint8_t *src_cb, const uint8_t *src_cr, uint32_t stride_c,
                                const SvtAmdOisLcuResult *ois, const SvtAmdMeLcuResult *me, const SvtAmdTmvpLcu *tmvp, const SvtAmdRefPicture *ref0,
                                const SvtAmdRefPicture *ref1, SvtAmdMdLcuOut *out, uint8_t *md_rec, uint8_t *ep_kind);
/* md_logic.h's motion-vector candidate lists and predictor choice on single units (pool: the motion-field records the jobs index) */
void svt_oracle_md_lists(const SvtAmdMdListJob *jobs, const SvtAmdTmvpLcu *pool, SvtAmdMdListOut *outs, int n);

/* The coding-unit loop of EncodePass for an LCU of intra 2Nx2N units (svt_oracle_encodepass.c): picture state in / out */
void svt_oracle_encode_lcu(uint8_t *const rec[3], const uint32_t pitch[3], uint8_t *map, uint32_t mapPitch, uint32_t width, uint32_t height,
                           const SvtAmdLcuWork *W, SvtAmdLcuResult *R);
void svt_oracle_encode_lcu16(uint16_t *const rec[3], const uint32_t pitch[3], uint8_t *map, uint32_t mapPitch, uint32_t width, uint32_t height,
                             const SvtAmdLcuWork16 *W, SvtAmdLcuResult16 *R);
void svt_oracle_encode_lcu_inter(uint8_t *const rec[3], const uint32_t pitch[3], uint8_t *map, uint32_t mapPitch, uint32_t width, uint32_t height,
                                 const SvtAmdRefPicture *ref0, const SvtAmdRefPicture *ref1, const SvtAmdCabacCost *cost, const SvtAmdLcuWork *W,
                                 SvtAmdLcuResult *R);
void svt_oracle_encode_lcu_inter16(uint16_t *const rec[3], const uint32_t pitch[3], uint8_t *map, uint32_t mapPitch, uint32_t width, uint32_t height,
                                   const SvtAmdRefPicture *ref0, const SvtAmdRefPicture *ref1, const SvtAmdCabacCost *cost, const SvtAmdLcuWork16 *W,
                                   SvtAmdLcuResult16 *R);

/* ---- entropy hand-off pre-scan (svt_oracle_coeffscan.c): the part of EncodeQuantizedCoefficients before the first bin ---- */
void svt_oracle_coeff_scan_tu(const int16_t *coeff, uint32_t stride, uint32_t size, uint32_t type, uint32_t intra_luma_mode, int is_chroma,
                              uint32_t nz, SvtAmdCoeffScanTu *tu, SvtAmdCoeffScanGroup *groups, uint32_t *ng, uint16_t *levels, uint32_t *nl);
int svt_oracle_coeff_scan_lcu(const SvtAmdLcuWork *W, const SvtAmdLcuResult *R, SvtAmdCoeffScanLcu *out, SvtAmdCoeffScanGroup *groups, uint16_t *levels);

/* ---- source-based operations: AC energy of the LCUs (svt_oracle_sbo.c) ---- */
uint64_t svt_oracle_sbo_ac_energy(const uint8_t *src, uint32_t stride, uint32_t width, uint32_t height);
void svt_oracle_sbo_ac_energy_picture(const uint8_t *luma, uint32_t stride, uint32_t width, uint32_t height, uint64_t *out);

/* ---- picture-analysis statistics (svt_oracle_pa.c) ---- */
void svt_oracle_pa_block_stats(const uint8_t *luma, uint32_t stride, SvtAmdPaLcuStats *out);
uint64_t svt_oracle_pa_luma_histogram(const uint8_t *sixteenth, uint32_t stride, uint32_t width, uint32_t height, uint32_t regions_w, uint32_t regions_h,
                                      uint32_t *histogram, uint8_t *region_average);

#endif
