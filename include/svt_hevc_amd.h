/*
 * svt_hevc_amd.h - C-ABI of the MI355X-native block-analysis hot path of SVT-HEVC.
 *
 * Two layers:
 *
 *  (1) LEAF layer ("svt_amd_<ReferenceName>"): one entry point per slot of the
 *      reference's [EB_ASM_TYPE_TOTAL] function-pointer tables, with the exact
 *      argument list of the reference typedef it replaces, on HOST pointers,
 *      synchronous.  A maintainer drops these into a third table slot
 *      (INTEGRATION.md).  They exist for per-call differential parity, not speed.
 *
 *  (2) BATCHED layer: one call per picture for the open-loop front half
 *      (pad + decimate + HME L0/L1/L2 + full-pel 85-PU search + AVC-style
 *      half/quarter-pel refinement + bi-pred + candidate sort), called from
 *      MotionEstimationKernel in place of its LCU loop
 *      (reference: Source/Lib/Codec/EbMotionEstimationProcess.c:706-820).
 *      Device state lives behind an opaque handle.
 *
 * Plain C types only.  All functions return 0 (SVT_AMD_OK) or a negative
 * SvtAmdStatus; nothing here falls back to a CPU implementation - if the HIP
 * device or code object is unavailable the call fails with SVT_AMD_ERR_DEVICE.
 */
#ifndef SVT_HEVC_AMD_H
#define SVT_HEVC_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_AMD_API __attribute__((visibility("default")))

typedef enum SvtAmdStatus {
    SVT_AMD_OK = 0,
    SVT_AMD_ERR_BAD_PARAM = -1,   /* maps to EB_ErrorBadParameter            (EbApi.h:114-129) */
    SVT_AMD_ERR_RESOURCES = -2,   /* maps to EB_ErrorInsufficientResources                     */
    SVT_AMD_ERR_DEVICE = -3       /* HIP failure; maps to EB_ErrorUndefined                    */
} SvtAmdStatus;

/* ------------------------------------------------------------------------- */
/* Shared data model                                                         */
/* ------------------------------------------------------------------------- */

#define SVT_AMD_LCU_SIZE 64
#define SVT_AMD_ME_PU_COUNT 85        /* MAX_ME_PU_COUNT, EbMotionEstimationLcuResults.h:14 */
#define SVT_AMD_PAD_FULL 68           /* lcuSize + ME_FILTER_TAP, EbEncHandle.c:901-904     */
#define SVT_AMD_PAD_QUARTER 32        /* EbEncHandle.c:911-914                              */
#define SVT_AMD_PAD_SIXTEENTH 16      /* EbEncHandle.c:921-924                              */

/* fractionalSearchMethod values, EbDefinitions.h:756-758 */
#define SVT_AMD_SUB_SAD_SEARCH 0
#define SVT_AMD_FULL_SAD_SEARCH 1
#define SVT_AMD_SSD_SEARCH 2

/* prediction direction, EbDefinitions.h (UNI_PRED_LIST_0/1, BI_PRED) */
#define SVT_AMD_UNI_PRED_LIST_0 0
#define SVT_AMD_UNI_PRED_LIST_1 1
#define SVT_AMD_BI_PRED 2

/*
 * Per-picture ME/HME controls.  Every field is a value the reference derives
 * on the host (out of the hot-path scope) and hands to MotionEstimateLcu:
 *   MeContext_t fields set by SetMeHmeParamsOq / SignalDerivationMeKernelOq
 *   (EbMotionEstimationProcess.c:54-120, 310-421) and PictureParentControlSet_t
 *   fields set by PictureDecision (EbPictureDecisionProcess.c:334-470).
 */
typedef struct SvtAmdMeParams {
    uint16_t luma_width;            /* SequenceControlSet_t.lumaWidth  (multiple of 8) */
    uint16_t luma_height;           /* SequenceControlSet_t.lumaHeight                  */
    uint8_t  num_lists;             /* 1: P picture (list 0 only), 2: B picture         */
    uint8_t  temporal_layer_index;  /* pcs->temporalLayerIndex                          */
    uint8_t  ref_pocs_equal;        /* refPicPocArray[0] == refPicPocArray[1]           */
    uint8_t  enable_hme_flag;       /* pcs->enableHmeFlag                               */
    uint8_t  enable_hme_level0;     /* pcs->enableHmeLevel0Flag                         */
    uint8_t  enable_hme_level1;
    uint8_t  enable_hme_level2;
    uint8_t  one_quadrant_hme;      /* MeContext_t.oneQuadrantHME                       */
    uint8_t  update_hme_search_center; /* MeContext_t.updateHmeSearchCenter             */
    uint8_t  num_hme_regions_w;     /* numberHmeSearchRegionInWidth  (<= 2)             */
    uint8_t  num_hme_regions_h;     /* numberHmeSearchRegionInHeight (<= 2)             */
    uint8_t  search_area_width;     /* MeContext_t.searchAreaWidth  (full-pel)          */
    uint8_t  search_area_height;
    uint8_t  fractional_search_method; /* SVT_AMD_*_SEARCH                              */
    uint8_t  fractional_search_model;  /* 0: all, 1: SuPelEnable gated, 2: off          */
    uint8_t  fractional_search_64x64;
    uint8_t  cu8x8_mode;            /* pcs->cu8x8Mode  (1 = no 8x8 refinement/bipred)   */
    uint8_t  cu16x16_mode;          /* pcs->cu16x16Mode                                 */
    uint16_t hme_l0_total_w;        /* hmeLevel0TotalSearchAreaWidth                    */
    uint16_t hme_l0_total_h;
    uint16_t hme_l0_w[2];           /* hmeLevel0SearchAreaInWidthArray                  */
    uint16_t hme_l0_h[2];
    uint16_t hme_l1_w[2];
    uint16_t hme_l1_h[2];
    uint16_t hme_l2_w[2];
    uint16_t hme_l2_h[2];
    uint16_t hme_l0_mult_x;         /* HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_X[hl][tl], EbDefinitions.h:1322 */
    uint16_t hme_l0_mult_y;
    uint32_t lambda;                /* MeContext_t.lambda (SAD lambda, EbMotionEstimationProcess.c:690-698) */
    uint32_t mvd_bits[12];          /* MeContext_t.mvdBitsArray (NUMBER_OF_MVD_CASES)   */
} SvtAmdMeParams;

/* One ME candidate record per PU; same content as MeCuResults_t
 * (EbMotionEstimationLcuResults.h:58-74) with explicit widths. */
typedef struct SvtAmdMeCuResult {
    int16_t  x_mv_l0, y_mv_l0, x_mv_l1, y_mv_l1;   /* quarter-pel units */
    uint32_t distortion[3];                          /* sorted candidates */
    uint8_t  direction[3];
    uint8_t  total_me_candidate_index;
} SvtAmdMeCuResult;

/* Full per-LCU output of the front half (what MotionEstimateLcu leaves behind). */
typedef struct SvtAmdMeLcuResult {
    SvtAmdMeCuResult pu[SVT_AMD_ME_PU_COUNT];        /* raster-within-tier order = meResults[lcu][pu] */
    uint32_t best_sad[2][SVT_AMD_ME_PU_COUNT];       /* pLcuBestSad[list][0][], internal Z order      */
    uint32_t best_mv[2][SVT_AMD_ME_PU_COUNT];        /* pLcuBestMV, (y<<16)|x quarter-pel             */
    int16_t  hme_center_x[2], hme_center_y[2];       /* search centre fed to the full-pel search      */
    int16_t  search_origin_x[2], search_origin_y[2]; /* x/ySearchAreaOrigin[list][0]                  */
    uint8_t  search_w[2], search_h[2];               /* clipped search area                           */
} SvtAmdMeLcuResult;

/* ------------------------------------------------------------------------- */
/* BATCHED layer                                                             */
/* ------------------------------------------------------------------------- */

typedef struct SvtAmdContext SvtAmdContext;          /* opaque; owns device, stream, arenas */

/* Library/device bring-up.  Replaces nothing in the reference: called from
 * EbInitEncoder/EbDeinitEncoder (EbEncHandle.c:689,1519) by the hook overlay. */
SVT_AMD_API int svt_amd_context_create(int device_ordinal, uint16_t max_luma_width,
                                       uint16_t max_luma_height, int num_picture_slots,
                                       SvtAmdContext **out_ctx);
SVT_AMD_API void svt_amd_context_destroy(SvtAmdContext *ctx);
SVT_AMD_API const char *svt_amd_version(void);
/* OPT-IN process setting for hosts that keep MORE streams in flight than the runtime's hardware queues (four by default; lanes = HIP streams, and
 * a context or lane holds a stream only from its first stream-ordered call on, see svt_amd_context_fork): asks the HIP runtime for 24 hardware queues
 * (GPU_MAX_HW_QUEUES, unless the user set it) so that every lane's stream has a queue of its own.  Only has an effect BEFORE the process's first
 * HIP call; the library never changes the environment on its own.  A host with up to three lanes beside the process's null stream does not need it. */
SVT_AMD_API int svt_amd_runtime_env_defaults(void);
/* OPT-IN device setting for hosts whose threads wait on the device while OTHER host threads have work to do (the encoder binding: up to a dozen EncDec threads
 * wait 60 - 100 ms each for their picture's mode-decision kernel while the base-layer pictures are decided on the same 32 logical processors): the threads sleep
 * in the HIP runtime's waits (hipDeviceScheduleBlockingSync) instead of spinning on a completion signal, which costs every wait a wake-up (tens of microseconds)
 * and gives the cores back.  blocking = 0 restores the runtime's default.  A setting of the DEVICE, i.e. of every context of this process on it; best made before
 * the device's first context (svt_amd_context_create). */
SVT_AMD_API int svt_amd_host_wait_mode(int device_ordinal, int blocking);
SVT_AMD_API const char *svt_amd_last_error(void);

/*
 * Upload one source luma plane into picture slot `slot` and build, on the
 * device, everything the PA reference object holds for ME:
 *   padded full-resolution plane      (GeneratePadding,   EbMcp.c:1017)
 *   1/4 and 1/16 point-decimated planes + their padding
 *                                     (DecimateInputPicture, EbPictureAnalysisProcess.c:4139;
 *                                      Decimation2D :173)
 *   AVC-style half-pel planes b, h, j (EbHevcInterpolateSearchRegionAVC, EbMotionEstimation.c:645;
 *                                      AvcStyleLumaInterpolationFilterHorizontal/Vertical,
 *                                      C_DEFAULT/EbAvcStyleMcp_C.c:34,62), computed once per picture
 *                                      instead of once per LCU per list.
 * `luma` is a HOST pointer to width x height samples with `stride` bytes per row.
 */
SVT_AMD_API int svt_amd_picture_upload(SvtAmdContext *ctx, int slot, const uint8_t *luma,
                                       uint32_t stride, uint16_t width, uint16_t height);

/* Same, but the plane already lives in device memory (bench / multi-GPU path). */
SVT_AMD_API int svt_amd_picture_upload_device(SvtAmdContext *ctx, int slot, const void *d_luma,
                                              uint32_t stride, uint16_t width, uint16_t height);
/* Up to 256 pictures of the same geometry in ONE launch (slots[i] <- d_luma[i]). */
SVT_AMD_API int svt_amd_picture_upload_device_batch(SvtAmdContext *ctx, int num, const int *slots,
                                                    const void *const *d_luma, uint32_t stride,
                                                    uint16_t width, uint16_t height);

/*
 * Motion estimation of one whole picture (all LCUs), replaces the LCU loop of
 * MotionEstimationKernel (EbMotionEstimationProcess.c:706-820) and
 * MotionEstimateLcu (EbMotionEstimation.c:3671-4450).
 *   cur_slot          picture being coded
 *   ref_slot[l]       PA reference picture of list l (ref_slot[1] ignored for P)
 *   out               HOST array of picWidthInLcu*picHeightInLcu records, raster LCU order
 * Blocking: returns when `out` is filled.
 */
SVT_AMD_API int svt_amd_me_picture(SvtAmdContext *ctx, const SvtAmdMeParams *params,
                                   int cur_slot, const int ref_slot[2],
                                   SvtAmdMeLcuResult *out);

/* Asynchronous form: results stay in device memory (slot-owned buffer) until
 * svt_amd_me_picture_fetch copies them out.  Used by bench.py and by a host
 * that overlaps ME of picture n+1 with EncDec of picture n. */
SVT_AMD_API int svt_amd_me_picture_launch(SvtAmdContext *ctx, const SvtAmdMeParams *params,
                                          int cur_slot, const int ref_slot[2]);
SVT_AMD_API int svt_amd_me_picture_fetch(SvtAmdContext *ctx, int cur_slot, SvtAmdMeLcuResult *out);
/*
 * Batched form: motion estimation of up to 256 pictures in ONE launch (grid = pictures x LCUs).
 * The front half is open loop, so every picture whose source and reference pictures have been
 * uploaded can be searched at once; this is what fills the 256 CUs (a single 1080p picture is
 * only 510 workgroups).  Results land in each current slot's result buffer (svt_amd_me_picture_fetch).
 * Reference analogue: several pictures are in flight across the 60 ME segment tasks per picture
 * (EbEncHandle.c:1680-1681, pictureControlSetPoolInitCount :1796-1809).
 */
typedef struct SvtAmdMeJob {
    SvtAmdMeParams params;
    int32_t cur_slot;
    int32_t ref_slot[2];
} SvtAmdMeJob;
SVT_AMD_API int svt_amd_me_batch_launch(SvtAmdContext *ctx, const SvtAmdMeJob *jobs, int num_jobs);

/* LCU-range form for multi-GPU sharding of one picture by LCU rows: only
 * records [lcu_begin, lcu_end) of the slot's result buffer are written.  The reference's
 * analogue is the 6x10 ME segment grid (EbEncHandle.c:1680-1681). */
SVT_AMD_API int svt_amd_me_picture_range_launch(SvtAmdContext *ctx, const SvtAmdMeParams *params,
                                                int cur_slot, const int ref_slot[2],
                                                uint32_t lcu_begin, uint32_t lcu_end);
SVT_AMD_API int svt_amd_synchronize(SvtAmdContext *ctx);
/* plain device memory on the context's GPU for C hosts that keep reference pictures / planes resident (blocking copies) */
SVT_AMD_API int svt_amd_device_alloc(SvtAmdContext *ctx, size_t bytes, void **d_ptr);
SVT_AMD_API int svt_amd_device_free(SvtAmdContext *ctx, void *d_ptr);
SVT_AMD_API int svt_amd_device_copy(SvtAmdContext *ctx, void *d_dst, const void *d_src, size_t bytes); /* device to device, blocking */
SVT_AMD_API int svt_amd_device_upload(SvtAmdContext *ctx, void *d_dst, const void *src, size_t bytes);
SVT_AMD_API int svt_amd_device_download(SvtAmdContext *ctx, void *dst, const void *d_src, size_t bytes);

/*
 * Open-loop intra search (OIS) of one whole picture: replaces the second LCU loop of
 * MotionEstimationKernel (EbMotionEstimationProcess.c:786-797) and OpenLoopIntraSearchLcu
 * (EbMotionEstimation.c:5053-5320): per 32x32 / 16x16 / 8x8 CU of every LCU, predict from SOURCE
 * neighbours (UpdateNeighborSamplesArrayOpenLoop, EbIntraPrediction.c:5222; out-of-picture = 128, no
 * smoothing) for the mode subset the slice type / OIS point selects, NxM SAD, candidate injection.
 */
typedef struct SvtAmdOisParams {
    uint16_t luma_width, luma_height;          /* SequenceControlSet_t.lumaWidth/Height                   */
    uint8_t  slice_is_intra;                   /* pcs->sliceType == EB_I_PICTURE                          */
    uint8_t  temporal_layer_index;             /* pcs->temporalLayerIndex                                 */
    uint8_t  limit_ois_to_dc_mode;             /* pcs->limitOisToDcModeFlag (EbPictureDecisionProcess.c:417) */
    uint8_t  skip_ois_8x8;                     /* pcs->skipOis8x8 (:455)                                  */
    uint8_t  cu8x8_mode;                       /* pcs->cu8x8Mode                                          */
    uint8_t  ois_kernel_level;                 /* MotionEstimationContext_t.oisKernelLevel (EbMotionEstimationProcess.c:356) */
    uint8_t  ois_th_set;                       /* .oisThSet (:371-393)                                    */
    uint8_t  set_best_ois_distortion_to_valid; /* .setBestOisDistortionToValid (:396)                     */
} SvtAmdOisParams;

#define SVT_AMD_OIS_MAX_CAND 18                /* MAX_OIS_2, EbCodingUnit.h:61 */
/* candidate word = OisCandidate_t.oisResults (EbCodingUnit.h:91-101): bits 0-19 distortion, 20 validDistortion,
 * 24-31 intraMode.  The reference only touches some bitfields of some entries per call (the rest keeps whatever
 * the PCS pool held); the three bits the reference leaves unnamed say which: */
#define SVT_AMD_OIS_W_DIST  (1u << 21)         /* this call wrote .distortion      */
#define SVT_AMD_OIS_W_VALID (1u << 22)         /* this call wrote .validDistortion */
#define SVT_AMD_OIS_W_MODE  (1u << 23)         /* this call wrote .intraMode       */
typedef struct SvtAmdOisLcuResult {
    uint32_t candidate[SVT_AMD_ME_PU_COUNT][SVT_AMD_OIS_MAX_CAND]; /* by rasterScanCuIndex; [0] (64x64) unused  */
    uint8_t  total_intra_luma_mode[SVT_AMD_ME_PU_COUNT];           /* 0xFF = left untouched by this call        */
    uint8_t  pad[3];
} SvtAmdOisLcuResult;
/* me: HOST array of the picture's ME results (distortion[0] of PUs 1..84 is read) or NULL - then the results of the
 * last ME launch for cur_slot, still resident on the device, are used (NULL is also right for I pictures and
 * limit_ois_to_dc_mode).  out: HOST array, one record per LCU, raster order.  Blocking. */
SVT_AMD_API int svt_amd_ois_picture(SvtAmdContext *ctx, const SvtAmdOisParams *params, int cur_slot,
                                    const SvtAmdMeLcuResult *me, SvtAmdOisLcuResult *out);
SVT_AMD_API int svt_amd_ois_picture_launch(SvtAmdContext *ctx, const SvtAmdOisParams *params, int cur_slot);
SVT_AMD_API int svt_amd_ois_picture_fetch(SvtAmdContext *ctx, int cur_slot, SvtAmdOisLcuResult *out);
/*
 * Collocated zero-motion SAD at 1/16 resolution and the background classes derived from it: replaces
 * ComputeDecimatedZzSad (EbMotionEstimationProcess.c:176-300, called per ME segment at :828 when lookAheadDistance != 0
 * and pictureNumber > 0).  prev_slot = the previous picture in display order; results are what the reference stores
 * into the PREVIOUS picture's zzCostArray / nonMovingIndexArray.  out: HOST array, one record per LCU.  Blocking.
 * Batched, stream-ordered form (results stay on the device): svt_amd_side_stats_batch_launch.
 */
typedef struct SvtAmdZzLcu {
    uint32_t sad;              /* decimatedLcuCollocatedSad (0xFFFFFFFF for incomplete LCUs)     */
    uint8_t  zz_cost;          /* zzCostArray[lcu]: 0 / 3 / 10 / 20 / 30, 0xFF = INVALID_ZZ_COST */
    uint8_t  non_moving_index; /* nonMovingIndexArray[lcu]: 0 / 10 / 20 / 30                     */
    uint8_t  pad[2];
} SvtAmdZzLcu;
SVT_AMD_API int svt_amd_zz_sad_picture(SvtAmdContext *ctx, int cur_slot, int prev_slot, SvtAmdZzLcu *out);

/*
 * Front-end pipeline (the asynchronous product path of the batched boundary `hip_me_picture`): replaces, per
 * picture, the LCU loops of MotionEstimationKernel (Codec/EbMotionEstimationProcess.c:706-820) with
 *     upload (pinned staging, asynchronous H2D) -> plane building -> ME of both lists -> OIS -> results into pinned host
 *     memory (asynchronous D2H)
 * queued on ONE stream ("lane") and overlapped with the other lanes' copies and kernels.  A lane is a context forked from
 * the one that owns the picture slots (svt_amd_context_fork): all lanes see the same slots, each has its own stream,
 * descriptors, timers and pinned result buffers.  The owning context is itself a lane.  Calls on one lane are serialised by
 * the caller; different lanes may be driven from different threads.  Destroy every lane before the owner: a lane's destructor waits for
 * the lane's work and then visits the owner's slots (it takes back the completion markers its ME / OIS launches lent them).
 * A context - the owner or a lane - takes its stream at its first stream-ordered call (a launch, an asynchronous copy or upload, a
 * lane event, a timer), not when it is made: an owner that only allocates (svt_amd_device_alloc, svt_amd_host_alloc), copies blocking
 * (svt_amd_device_upload / _download / _copy) and forks holds none, and svt_amd_synchronize of it returns at once.  Streams beyond the
 * runtime's hardware queues (four by default) share one and run in submission order with their neighbour, so what counts is the number
 * of contexts that queue work: three lanes under such an owner run side by side at the default (svt_amd_runtime_env_defaults for more).
 *   svt_amd_picture_upload_async  copies `luma` into pinned staging before returning (caller may reuse it), queues the rest
 *   svt_amd_frontend_submit       queues ME (has_me) and/or OIS (has_ois) of cur_slot + the result copies; never blocks
 *   svt_amd_frontend_wait         blocks until the lane's job is complete; *me / *ois point at the lane's pinned buffers
 *                                 (one record per LCU, raster order), valid until svt_amd_frontend_release
 */
typedef struct SvtAmdFrontendJob {
    int32_t cur_slot;
    int32_t ref_slot[2];
    uint8_t has_me;            /* P / B pictures */
    uint8_t has_ois;
    uint8_t compact;           /* 1: the lane's pinned buffers receive the COMPACT records (below) instead of the full ones */
    uint8_t pad;
    SvtAmdMeParams me;
    SvtAmdOisParams ois;
} SvtAmdFrontendJob;
SVT_AMD_API int svt_amd_context_fork(SvtAmdContext *parent, SvtAmdContext **out_lane);
SVT_AMD_API int svt_amd_picture_upload_async(SvtAmdContext *lane, int slot, const uint8_t *luma, uint32_t stride,
                                             uint16_t width, uint16_t height);
SVT_AMD_API int svt_amd_picture_publish(SvtAmdContext *lane, int slot);
SVT_AMD_API int svt_amd_frontend_submit(SvtAmdContext *lane, const SvtAmdFrontendJob *job);
SVT_AMD_API int svt_amd_frontend_wait(SvtAmdContext *lane, const SvtAmdMeLcuResult **me, const SvtAmdOisLcuResult **ois);
SVT_AMD_API int svt_amd_frontend_release(SvtAmdContext *lane);
/* Cross-lane ordering without host waits (for hosts that build their own copy-in -> compute -> copy-out pipelines): a lane records
 * its event `index` (0..7) at the current end of its stream; another lane's stream waits for the latest record of it. */
SVT_AMD_API int svt_amd_lane_event_record(SvtAmdContext *lane, int index);
SVT_AMD_API int svt_amd_lane_event_wait(SvtAmdContext *lane, SvtAmdContext *source, int index);
/* Compact wire format of the records (what the reference side of the boundary consumes; the full records also carry the internal
 * best-SAD / MV arrays and 18 candidate slots per CU for parity tests): per LCU
 *   ME :  SvtAmdMeCuResult[85]                                                        (2,040 B instead of 3,420)
 *   OIS:  uint32_t candidate[85][nc] + uint8_t total_intra_luma_mode[85] + 3 pad      (85 * nc * 4 + 88 B instead of 6,208)
 * nc = svt_amd_ois_compact_candidates(params) = the most candidates the picture's path writes per CU: 7 on I pictures, 9 on P / B
 * pictures, 18 with ois_kernel_level (MAX_OIS_0 / _1 / _2, Codec/EbCodingUnit.h:59-61).  The device packs, then copies. */
#define SVT_AMD_OIS_COMPACT_BYTES(nc) (SVT_AMD_ME_PU_COUNT * (nc) * 4 + 88)
SVT_AMD_API int svt_amd_ois_compact_candidates(const SvtAmdOisParams *params);
SVT_AMD_API int svt_amd_me_picture_fetch_compact_async(SvtAmdContext *ctx, int cur_slot, SvtAmdMeCuResult *out);
SVT_AMD_API int svt_amd_ois_picture_fetch_compact_async(SvtAmdContext *ctx, int cur_slot, int candidates, void *out);
/* n pictures at once (batched hosts): the slots' records packed into contiguous DEVICE arrays, picture i of the batch at index i of
 * d_me (LCUs x 85 records each) / d_ois (LCUs x SVT_AMD_OIS_COMPACT_BYTES(candidates) bytes each); either may be NULL.  Run it on
 * the lane that ran the searches and move the arrays with one copy each on any lane (svt_amd_device_download_async). */
SVT_AMD_API int svt_amd_records_pack_batch_async(SvtAmdContext *ctx, const int *slots, int n, int candidates, SvtAmdMeCuResult *d_me,
                                                 void *d_ois);
/* Start-up, outside any timed run: pins the staging buffers of every picture slot (root) and the lane's result buffers, and sends
 * one dummy picture through upload -> planes -> ME -> OIS so that the kernels' code objects are loaded.  Once per lane (and root). */
SVT_AMD_API int svt_amd_frontend_warmup(SvtAmdContext *ctx);
/* building blocks of the same pipeline for batched hosts (bench.py): stream-ordered copies that do not wait, pinned host
 * memory to copy from / into, and the per-slot result copies; svt_amd_synchronize(lane) completes them */
SVT_AMD_API int svt_amd_device_upload_async(SvtAmdContext *ctx, void *d_dst, const void *src, size_t bytes);
SVT_AMD_API int svt_amd_device_download_async(SvtAmdContext *ctx, void *dst, const void *d_src, size_t bytes);
SVT_AMD_API int svt_amd_host_alloc(SvtAmdContext *ctx, size_t bytes, void **h_ptr);
SVT_AMD_API int svt_amd_host_free(SvtAmdContext *ctx, void *h_ptr);
/* Page-locks a buffer the CALLER owns (hipHostRegister) so that copies from / into it go through the DMA engines instead of the runtime's staged copy of pageable
 * memory - which is a shader (blit) kernel on this runtime and competes for compute units with the persistent mode-decision kernels.  For host buffers that live as long
 * as the encoder (the reference's input-picture and reference-picture pools, Codec/EbEncHandle.c:1794-1813): a process-wide table remembers (pointer, size), a second
 * call for the same range costs a lookup.  Returns SVT_AMD_OK also when the runtime refuses the range (the copies then take the pageable path as before).
 * svt_amd_host_unregister_all() releases every registration (before the caller frees the buffers). */
SVT_AMD_API int svt_amd_host_register(SvtAmdContext *ctx, const void *h_ptr, size_t bytes);
SVT_AMD_API int svt_amd_host_unregister_all(SvtAmdContext *ctx);
SVT_AMD_API int svt_amd_me_picture_fetch_async(SvtAmdContext *ctx, int cur_slot, SvtAmdMeLcuResult *out);
SVT_AMD_API int svt_amd_ois_picture_fetch_async(SvtAmdContext *ctx, int cur_slot, SvtAmdOisLcuResult *out);

/*
 * Multi-GPU exchange of the closed-loop half (SURVEY 8e "EncDec with tiles").  Tiles are independent inside a picture
 * (Codec/EbEntropyCoding.c:6346-6351, EbEncDecProcess.c:2743-2760), so rank r encodes a rectangle of whole tiles; motion vectors
 * of later pictures may cross tile borders (EbEncHandle.c:2757), so every FINISHED reference picture is all-gathered once
 * (after DLF / SAO, before it is padded and referenced: EbEncDecProcess.c:1806) - the only data-path collective.
 *   svt_amd_tile_partition: the reference's uniform tile grid (tileColStartLcu[c] = c * widthInLcu / cols,
 *     Codec/EbPictureControlSet.c:743-750) -> rank_rect[world] (luma samples; every rank a rectangle of whole tiles) and,
 *     optionally, tile_rank[tile_rows * tile_cols].  Host code, no device needed.
 *   svt_amd_comm_*: RCCL communicator of a context (one process per GPU; rank 0 makes the id, the host passes it round -
 *     torch.distributed / MPI / a file).  librccl is opened at run time.
 *   svt_amd_recon_exchange: pack own rectangle of Y / Cb / Cr (4:2:0) -> ncclAllGather -> unpack the others into the local planes;
 *     stream-ordered on the context's stream.  d_planes: device pointers to sample (0,0); pitches in bytes.
 *   svt_amd_recon_pack: the local halves alone (planes <-> slot r of a caller-owned buffer), for hosts with their own transport.
 */
typedef struct SvtAmdRect { uint16_t x, y, w, h; } SvtAmdRect;
typedef struct SvtAmdCommId { char bytes[128]; } SvtAmdCommId;
SVT_AMD_API int svt_amd_tile_partition(uint16_t luma_width, uint16_t luma_height, int tile_cols, int tile_rows, int world,
                                       SvtAmdRect *rank_rect, int *tile_rank);
SVT_AMD_API int svt_amd_comm_unique_id(SvtAmdCommId *out);
SVT_AMD_API int svt_amd_comm_init(SvtAmdContext *ctx, int world, int rank, const SvtAmdCommId *id);
SVT_AMD_API int svt_amd_comm_destroy(SvtAmdContext *ctx);
SVT_AMD_API int svt_amd_recon_exchange(SvtAmdContext *ctx, void *const d_planes[3], const uint32_t pitch_bytes[3], int bytes_per_sample,
                                       const SvtAmdRect *rects, int world, int rank);
SVT_AMD_API int svt_amd_recon_pack(SvtAmdContext *ctx, void *const d_planes[3], const uint32_t pitch_bytes[3], int bytes_per_sample,
                                   const SvtAmdRect *rects, int world, int r, void *d_slots, size_t slot_bytes, int to_slot);

/*
 * Picture-analysis statistics: what GatheringPictureStatistics (Codec/EbPictureAnalysisProcess.c:3995) computes from the planes the
 * front half already holds in HBM, one call per picture slot (after svt_amd_picture_upload*):
 *   per LCU  variance[85] / y_mean[85] of the 64x64, 32x32, 16x16 and 8x8 blocks in the order of the motion-estimation units
 *            (ME_TIER_ZERO_PU_*: 64x64, four 32x32, sixteen 16x16, sixty-four 8x8, each raster) - ComputeBlockMeanComputeVariance (:1646): sums and
 *            sums of squares over the EVEN rows of each 8x8 block, means in 8 / 16 fractional bits averaged up the tree with >> 2;
 *   per picture  the luma histograms of the regions_w x regions_h regions of the 1/16 picture (bins start at 1 and end << 4,
 *            SubSampleLumaGeneratePixelIntensityHistogramBins :3384), the regions' average intensity and the picture's luma sum (<< 4 per region).
 * out: HOST, LCUs of the picture in raster order; histogram: HOST [regions_w][regions_h][256] or NULL; region_average: HOST [regions_w][regions_h]
 * or NULL; sum_luma: HOST or NULL.  Blocking.
 * Batched, stream-ordered form (results stay on the device): svt_amd_side_stats_batch_launch.
 */
typedef struct SvtAmdPaLcuStats {
    uint16_t variance[SVT_AMD_ME_PU_COUNT];  /* pictureControlSetPtr->variance[lcu]  */
    uint8_t y_mean[SVT_AMD_ME_PU_COUNT];     /* pictureControlSetPtr->yMean[lcu]     */
    uint8_t pad;
} SvtAmdPaLcuStats;
SVT_AMD_API int svt_amd_picture_stats(SvtAmdContext *ctx, int slot, SvtAmdPaLcuStats *out, int regions_w, int regions_h, uint32_t *histogram,
                                      uint8_t *region_average, uint64_t *sum_luma);

/*
 * Source-based-operations input of the mode-decision configuration: CalculateAcEnergy (Codec/EbSourceBasedOperationsProcess.c:302-362) of
 * every LCU of the picture the slot holds - the AC energy (ComputeNxMSatdSadLCU, Codec/EbPictureOperators.c:232: 8x8 Hadamard sums minus the DC terms >> 2)
 * of the 64x64 and of its four 32x32, the values pictureControlSetPtr->lcuYSrcEnergyCuArray[lcu][0..4] carries into DeriveDefaultSegments
 * (EbModeDecisionConfiguration.c:409-426) and the encode pass's skin / contour tests (EbModeDecisionProcess.c:542).  LCUs the picture does not cover completely
 * get the reference's 100000000 (:351).  Which pictures the values are read for (I pictures outside low-delay P) is the caller's rule.
 * out: HOST, [LCUs in raster order][5].  Blocking.
 * Batched, stream-ordered form (results stay on the device): svt_amd_side_stats_batch_launch.
 */
SVT_AMD_API int svt_amd_picture_ac_energy(SvtAmdContext *ctx, int slot, uint64_t *out);

/* Batched form (grid = pictures x LCUs), each job reading the ME results its slot holds on the device. */
typedef struct SvtAmdOisJob {
    SvtAmdOisParams params;
    int32_t cur_slot;
} SvtAmdOisJob;
SVT_AMD_API int svt_amd_ois_batch_launch(SvtAmdContext *ctx, const SvtAmdOisJob *jobs, int num_jobs);

/*
 * Batched side statistics: the three per-picture results above that belong to the same stage as ME / OIS, for up to 256 pictures of ONE geometry per call,
 * stream-ordered on the context's lane like svt_amd_me_batch_launch / svt_amd_ois_batch_launch / svt_amd_records_pack_batch_async - the call never blocks and
 * never copies to the host:
 *   block_stats     ComputeBlockMeanComputeVariance (Codec/EbPictureAnalysisProcess.c:1646)      } one kernel, ONE read of the luma plane: a wave per LCU,
 *   ac_energy       CalculateAcEnergy (Codec/EbSourceBasedOperationsProcess.c:302-362;           } a lane per 8x8 block (svt_amd_picture_stats and
 *                   ComputeNxMSatdSadLCU, Codec/EbPictureOperators.c:232)                        } svt_amd_picture_ac_energy read it once each)
 *   histogram, region_average, sum_luma
 *                   SubSampleLumaGeneratePixelIntensityHistogramBins (Codec/EbPictureAnalysisProcess.c:3384) on the 1/16 pictures, regions_w x regions_h
 *                   regions (at most 64; only read when some job wants histograms); region_average and sum_luma are written for the pictures that want
 *                   histograms where those arrays are given, the bytes of a picture's region_average beyond its regions are 0
 *   zz              ComputeDecimatedZzSad (Codec/EbMotionEstimationProcess.c:176-300) of cur_slot against prev_slot: record i is what the reference stores into
 *                   the PREVIOUS picture's zzCostArray / nonMovingIndexArray, as for svt_amd_zz_sad_picture
 * Values are those of the three blocking entries, byte for byte.  The arrays are DEVICE memory (svt_amd_device_alloc), picture i of the batch at i times
 * svt_amd_side_stats_bytes(...) bytes of each; a picture that does not want a result leaves its part of that array untouched.  The histogram and sum_luma parts
 * the kernels accumulate into are zeroed by the call.  The call waits, on the device, for the planes of every slot it reads - each job's prev_slot included -
 * so they may have been built on another lane.  Move the results with svt_amd_device_download_async on any lane behind svt_amd_lane_event_record / _wait: one
 * copy per kind for the whole batch.  Everything is checked before anything is queued: a job that wants a result whose array is NULL, a slot that holds no
 * picture or one of another size than job 0's, or bad regions return SVT_AMD_ERR_BAD_PARAM (svt_amd_last_error says which) and queue nothing.
 */
typedef struct SvtAmdSideJob {
    int32_t cur_slot;
    int32_t prev_slot;          /* previous picture in display order; < 0: no zz-SAD for this picture */
    uint8_t want_block_stats, want_ac_energy, want_histogram, pad;
} SvtAmdSideJob;                /* 12 bytes */
typedef struct SvtAmdSideArrays {          /* DEVICE pointers, picture i of the batch at index i; any may be NULL */
    SvtAmdPaLcuStats *block_stats;         /* [n][lcus]            pictureControlSetPtr->variance / yMean (EbPictureAnalysisProcess.c:1646)  */
    uint64_t         *ac_energy;           /* [n][lcus][5]         lcuYSrcEnergyCuArray[lcu][0..4] (EbSourceBasedOperationsProcess.c:302)    */
    SvtAmdZzLcu      *zz;                  /* [n][lcus]            zzCostArray / nonMovingIndexArray (EbMotionEstimationProcess.c:176-300)   */
    uint32_t         *histogram;           /* [n][regions_w][regions_h][256]   pictureHistogram (EbPictureAnalysisProcess.c:3384)            */
    uint8_t          *region_average;      /* [n][regions_w][regions_h], each picture padded to 64 bytes   averageIntensityPerRegion (:3428) */
    uint64_t         *sum_luma;            /* [n]                  the sum CalculateInputAverageIntensity (:3953) divides                    */
} SvtAmdSideArrays;
SVT_AMD_API int svt_amd_side_stats_batch_launch(SvtAmdContext *ctx, const SvtAmdSideJob *jobs, int num_jobs, int regions_w, int regions_h,
                                                const SvtAmdSideArrays *out);
/* bytes ONE picture of luma_width x luma_height takes in array `which` (picture i of a batch starts at i times this); 0 for an unknown `which` or bad
 * regions.  Host arithmetic: no context, no device. */
#define SVT_AMD_SIDE_BLOCK_STATS 0
#define SVT_AMD_SIDE_AC_ENERGY   1
#define SVT_AMD_SIDE_ZZ          2
#define SVT_AMD_SIDE_HISTOGRAM   3
#define SVT_AMD_SIDE_REGION_AVG  4
#define SVT_AMD_SIDE_SUM_LUMA    5
SVT_AMD_API size_t svt_amd_side_stats_bytes(uint16_t luma_width, uint16_t luma_height, int which, int regions_w, int regions_h);

/*
 * Batched chroma statistics: the chroma half of GatheringPictureStatistics (Codec/EbPictureAnalysisProcess.c:3995) for up to 256 pictures of ONE geometry per
 * call, stream-ordered on the context's lane like svt_amd_side_stats_batch_launch - the call never blocks and never copies to the host.  A batch of one picture
 * is the single-picture form.
 *   means           ComputeChromaBlockMean (:1448) / ZeroOutChromaBlockMean (:1383): per LCU cb_mean[21] / cr_mean[21] in ME_TIER_ZERO_PU order (64x64, four
 *                   32x32, sixteen 16x16, each raster).  A 16x16 luma unit is an 8x8 chroma block; its mean is ComputeSubMean8x8_SSE2_INTRIN
 *                   (ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c:53): the sum of rows 0, 2, 4 and 6 << 3, MEAN_PRECISION (8) fractional bits; 32x32 and 64x64 are averaged
 *                   up the tree with >> 2.  As in the reference, the 64x64 mean adds 32x32 block 3 twice and never reads block 2 (:1586-1587).  LCUs the picture
 *                   does not cover completely get zeros.  One wave per LCU, a lane per 8x8 chroma block of one plane (v_sad_u8), the tree by lane shuffles.
 *   histogram, region_average, sum_chroma
 *                   SubSampleChromaGeneratePixelIntensityHistogramBins (:3440) with CalculateHistogram (:204) at decimStep 4: regions are cut on the LUMA
 *                   dimensions (width / regions_w, the remainder to the last region); the chroma origin is the luma region origin >> 1 and the area the luma
 *                   region size >> 1; every 4th sample of every 4th row is counted; bins start at 1, bins and sums end << 4.  region_average has the rounding
 *                   of :3491 (divisor area >> 2, rounding term area >> 3, truncated to a byte); sum_chroma holds the two sums CalculateInputAverageIntensity
 *                   (:3983-3984) divides.  Index 0 of every [2] is Cb, 1 is Cr.
 * cb / cr: DEVICE pointers to sample (0,0) of the 8-bit, unpadded 4:2:0 planes of the input picture (luma_width / 2 x luma_height / 2 samples, `pitch` bytes a
 * row for both, any alignment).  The caller puts them there (svt_amd_device_upload_async) or already has them; picture slots are not touched, and ORDERING AGAINST
 * WHATEVER WROTE THE PLANES IS THE CALLER'S: queue the call on the lane that wrote them, or behind svt_amd_lane_event_record / _wait.  A job that wants
 * neither result reads no plane (cb / cr may be NULL).  The arrays are DEVICE memory, picture i of the batch at i times svt_amd_chroma_stats_bytes(...) bytes of each; a picture that does not want a result
 * leaves its part of that array untouched; the histogram and sum_chroma parts the kernels accumulate into are zeroed by the call.  Everything is checked before
 * anything is queued: a job that wants a result whose array is NULL, a plane pointer without the other, a pitch below luma_width / 2, odd or zero dimensions, or
 * regions that do not fit (more than 64, or a region below 8 luma samples a side) return SVT_AMD_ERR_BAD_PARAM (svt_amd_last_error names the job) and queue nothing.
 */
typedef struct SvtAmdPaLcuChroma {
    uint8_t cb_mean[21];        /* pictureControlSetPtr->cbMean[lcu][0..20] */
    uint8_t cr_mean[21];        /* pictureControlSetPtr->crMean[lcu][0..20] */
    uint8_t pad[6];             /* 0 */
} SvtAmdPaLcuChroma;            /* 48 bytes */
typedef struct SvtAmdChromaJob {
    const uint8_t *cb, *cr;     /* DEVICE; only read when the job wants a result */
    uint32_t pitch;             /* bytes a row, both planes */
    uint8_t want_means, want_histogram, pad[2];
} SvtAmdChromaJob;              /* 24 bytes */
typedef struct SvtAmdChromaArrays {        /* DEVICE pointers, picture i of the batch at index i; any may be NULL */
    SvtAmdPaLcuChroma *means;              /* [n][lcus]                           cbMean / crMean (EbPictureAnalysisProcess.c:1448)          */
    uint32_t          *histogram;          /* [n][regions_w][regions_h][2][256]   pictureHistogram[..][..][1..2] (:3440)                     */
    uint8_t           *region_average;     /* [n][64][2], regions in [regions_w][regions_h] order, the rest 0   averageIntensityPerRegion[..][..][1..2] (:3491) */
    uint64_t          *sum_chroma;         /* [n][2]                              sumAverageIntensityTotalRegionsCb / Cr (:3490, :3983-3984) */
} SvtAmdChromaArrays;
SVT_AMD_API int svt_amd_chroma_stats_batch_launch(SvtAmdContext *ctx, const SvtAmdChromaJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                  int regions_w, int regions_h, const SvtAmdChromaArrays *out);
#define SVT_AMD_CHROMA_MEANS      0
#define SVT_AMD_CHROMA_HISTOGRAM  1
#define SVT_AMD_CHROMA_REGION_AVG 2
#define SVT_AMD_CHROMA_SUM        3
/* bytes ONE picture takes in array `which`; 0 for an unknown `which` or bad regions.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_chroma_stats_bytes(uint16_t luma_width, uint16_t luma_height, int which, int regions_w, int regions_h);

/*
 * Batched picture detectors: what ComputePictureSpatialStatistics (Codec/EbPictureAnalysisProcess.c:3879) derives from the block statistics, for up to 256 pictures of
 * ONE geometry per call, stream-ordered on the context's lane, never blocking, never copying to the host.  A batch of one picture is the single-picture form.
 *   stats           DEVICE, required: the SvtAmdPaLcuStats[lcus] svt_amd_side_stats_batch_launch left (same lane: no further ordering needed)
 *   chroma          DEVICE or NULL: the SvtAmdPaLcuChroma[lcus] of svt_amd_chroma_stats_batch_launch; required only with want_edge16
 *   want_edge16     the reference computes the 16x16 edge map only when (pictureNumber & 3) == 0 and clears it otherwise (:3535): that rule is the caller's
 *   resolution_class  SequenceControlSet_t.inputResolution (0 = 576p range or lower .. 3 = 4K range, Codec/EbSequenceControlSet.c:288): it selects the
 *                   potentialLogoLcu map, which is derived on the device from the geometry as Codec/EbSequenceControlSet.c:216-273 does
 * Per picture: pic_avg_variance (:3930-3933) = the sum of the 64x64 variances of ALL LCUs / the LCU count, truncated to 16 bits.
 * DetermineHomogeneousRegionInPicture (:3751): var_of_var_32x32 (all-ones for incomplete LCUs) and homogeneous (1 for incomplete LCUs); very_low_var_pic and
 * logo_pic are counted over complete LCUs only.  The squares of the 16-bit variances are summed in 64 bits, then >> 4 (32x32) / >> 6 (64x64); the subtraction is
 * unsigned 64-bit as written, so a mean square below the squared mean wraps.
 * EdgeDetection (:3627), restated as it is: edge_block_num (the 64x64 variance above 70 % of pic_avg_variance), sharp_edge (variance above 200 with more than four
 * 16x16 variances below 20) and lcu_block_percentage for LCUs with a neighbour on every side; the high-intensity test (mean above 180 next to a mean below 120)
 * for LCUs with four LCUs on every side.  isolated_high_intensity is ORDER-DEPENDENT in the reference: every LCU clears its own flag when the raster loop reaches it,
 * so the 9x9 mark a triggering LCU m sets on a later LCU n > m is wiped and one on n <= m stays.  The device gives that final state - the flag of n is 1 exactly
 * when some triggering LCU m >= n lies within +-4 LCU columns and rows of n - and does not repair it.
 * EdgeDetectionMeanLumaChroma16x16 (:3522): for complete potentialLogoLcu LCUs the gradient of the 16x16 means (Y, Cr, Cb; integer division by the number of
 * neighbours), maxGrad = the picture-wide maximum starting at 1, edge_cu bit i = min(grad * 765 / maxGrad, 255) >= 30; every other LCU gets 0, and every LCU gets 0
 * without want_edge16.
 * Three stages in stream order - per LCU (a lane per 8x8 variance, lane shuffles, 64-bit sums) with the picture reduction by vector atomics into a context-owned
 * scratch the call zeroes, then what needs the reduced values (per LCU, and a workgroup per picture for the 9x9 gather and the picture record).  Everything is checked before anything is queued: a NULL stats pointer, want_edge16 without chroma,
 * a resolution class above 3, a NULL output array or a picture of more than 16384 LCUs return SVT_AMD_ERR_BAD_PARAM (svt_amd_last_error names the job) and queue nothing.
 */
typedef struct SvtAmdPaLcuDetect {
    uint64_t var_of_var_32x32[4];       /* varOfVar32x32BasedLcuArray[lcu][0..3]; 0xFFFFFFFFFFFFFFFF for incomplete LCUs (:3850)   */
    uint16_t edge_cu;                   /* bit i: lcuStatArray[lcu].cuStatArray[RASTER_SCAN_CU_INDEX_16x16_0 + i].edgeCu (:3609)    */
    uint8_t  homogeneous;               /* lcuHomogeneousAreaArray[lcu] (:3774, :3842)                                              */
    uint8_t  edge_block_num;            /* edgeResultsPtr[lcu].edgeBlockNum (:3682)                                                 */
    uint8_t  isolated_high_intensity;   /* edgeResultsPtr[lcu].isolatedHighIntensityLcu after the whole raster loop (:3669, :3729)  */
    uint8_t  sharp_edge;                /* sharpEdgeLcuFlag[lcu] (:3691)                                                            */
    uint8_t  pad[10];                   /* 0 */
} SvtAmdPaLcuDetect;                    /* 48 bytes */
typedef struct SvtAmdPaPicDetect {
    uint16_t pic_avg_variance;          /* picAvgVariance (:3933)      */
    uint8_t  very_low_var_pic;          /* veryLowVarPicFlag (:3856)   */
    uint8_t  logo_pic;                  /* logoPicFlag (:3863)         */
    uint8_t  lcu_block_percentage;      /* lcuBlockPercentage (:3743)  */
    uint8_t  pad[3];                    /* 0 */
} SvtAmdPaPicDetect;                    /* 8 bytes */
typedef struct SvtAmdDetectJob {
    const SvtAmdPaLcuStats  *stats;     /* DEVICE [lcus], required */
    const SvtAmdPaLcuChroma *chroma;    /* DEVICE [lcus] or NULL   */
    uint8_t want_edge16, resolution_class, pad[6];
} SvtAmdDetectJob;                      /* 24 bytes */
typedef struct SvtAmdDetectArrays {     /* DEVICE pointers, picture i of the batch at index i; both required */
    SvtAmdPaLcuDetect *lcu;             /* [n][lcus] */
    SvtAmdPaPicDetect *picture;         /* [n]       */
} SvtAmdDetectArrays;
SVT_AMD_API int svt_amd_picture_detect_batch_launch(SvtAmdContext *ctx, const SvtAmdDetectJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                    const SvtAmdDetectArrays *out);
#define SVT_AMD_DETECT_LCU     0
#define SVT_AMD_DETECT_PICTURE 1
/* bytes ONE picture takes in array `which`; 0 for an unknown `which`.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_picture_detect_bytes(uint16_t luma_width, uint16_t luma_height, int which);

/*
 * Batched noise detection: what PicturePreProcessingOperations (Codec/EbPictureAnalysisProcess.c:3338) leaves behind for later stages - picNoiseClass and
 * lcuFlatNoiseArray - for up to 256 pictures of ONE geometry per call, stream-ordered on the context's lane like svt_amd_side_stats_batch_launch: the call never
 * blocks and never copies to the host.  A batch of one picture is the single-picture form.  enableDenoiseSrcFlag is EB_FALSE in every configuration of the
 * reference (Codec/EbResourceCoordinationProcess.c:304), so the denoise filters never run and the input picture is never rewritten: detection is all there is.
 *   method          the reference's EB_NOISE_DETECT_MODE: SVT_AMD_NOISE_FULL = DetectInputPictureNoise (:2539) on the input luma, 64x64 blocks;
 *                   SVT_AMD_NOISE_QUARTER = QuarterSampleDetectNoise (:2909) on the 1/4 picture, 32x32 blocks; SVT_AMD_NOISE_HALF = SubSampleDetectNoise (:3052)
 *                   on the 1/16 picture, 16x16 blocks.  A block stands for one LCU of the input picture.  The planes are those of the picture slot.
 *   noise_detection_th  the reference's noiseDetectionTh, 0 or 1: the noise variance of a flat-noise block must exceed 120000 (0) or 70000 (1).
 *                   Deriving method and threshold from encMode and the resolution class (Codec/EbResourceCoordinationProcess.c:248-284) is the caller's.
 * The weak luma filter (getFilteredTypes(.., 0), :956-961): denoised = (top + left + 4 * centre + right + bottom) / 8, noise = centre - denoised clamped at 0; the
 * first and last row and column of the plane the method reads are copied, with noise 0 (:1303-1312).  Block variances are ComputeVariance64x64 / 32x32 / 16x16
 * (:431, :231, :377): 8x8 means << 8 and means of squares << 16 (ComputeMeanFunc, Codec/EbComputeMean.h:25), averaged up the tree with >> 2, the subtraction
 * unsigned 64-bit as written.  A block is flat noise when its denoised variance >> 16 is below 50 and its noise variance exceeds the threshold.
 * The reference's noise picture is ONE 64-row strip reused for every block row (noiseOriginIndex has no vertical term: :2573, :2983, :3127).  In the two
 * decimated methods every vertically stacked 16x16 (32x32) block of a 64x64 block of the decimated picture therefore shares the noise variance of the TOP rows
 * of that 64x64 block, while its denoised variance comes from its own rows; restated as it is.  The full method evaluates complete LCUs only; the decimated
 * methods only the blocks inside floor(width / 64) x floor(height / 64) 64x64 blocks of the decimated picture (4K: the last two LCU rows are left out), so a
 * decimated picture below 64 samples a side evaluates nothing - block_count 0, sum 0, class 1, no flags - and is no error.
 * Class ladders on noise_variance_sum / block_count (integer), noiseTh by the slot's luma height: full (:2635-2664) noiseTh 25 up to 720 rows, else 0, rungs
 * 5 / 10 / 17 + noiseTh for classes 2 / 3 / 3_1, everything above folded to 3_1; half (:3171-3186) noiseTh 25 / 10 / 0 up to 720 / 1080 / above, rungs 5 / 10 / 55 +
 * noiseTh; quarter (:3032-3042) noiseTh 0, rungs 5 / 10 and the strict > 60.  picNoiseVarianceFloat (read by the dead denoiser only) is noise_variance_sum /
 * block_count, exactly, on the host; the device does no floating point.
 * The arrays are DEVICE memory, both required, picture i of the batch at i times svt_amd_noise_detect_bytes(...) bytes of each.  The call waits on the device for
 * the planes of every slot it reads, zeroes what it accumulates into, and checks everything before it queues anything: a NULL array, an unknown method, a
 * threshold above 1, a slot that holds no picture or one of another size than job 0's return SVT_AMD_ERR_BAD_PARAM (svt_amd_last_error names the job) and queue
 * nothing.
 */
#define SVT_AMD_NOISE_HALF    0         /* NOISE_DETECT_HALF_PRECISION    (Codec/EbDefinitions.h:1207) */
#define SVT_AMD_NOISE_QUARTER 1         /* NOISE_DETECT_QUARTER_PRECISION */
#define SVT_AMD_NOISE_FULL    2         /* NOISE_DETECT_FULL_PRECISION    */
typedef struct SvtAmdNoiseJob {
    int32_t cur_slot;
    uint8_t method;                     /* SVT_AMD_NOISE_* */
    uint8_t noise_detection_th;         /* 0 or 1 */
    uint8_t pad[2];
} SvtAmdNoiseJob;                       /* 8 bytes */
typedef struct SvtAmdNoisePic {
    uint64_t noise_variance_sum;        /* the sum of noiseBlkVar >> 16 over the evaluated blocks (:2612, :2991, :3135) */
    uint32_t block_count;               /* totLcuCount */
    uint8_t  pic_noise_class;           /* picNoiseClass: PIC_NOISE_CLASS_1 = 1, _2 = 2, _3 = 3, _3_1 = 4 */
    uint8_t  pad[3];                    /* 0 */
} SvtAmdNoisePic;                       /* 16 bytes */
typedef struct SvtAmdNoiseArrays {      /* DEVICE pointers, picture i of the batch at index i; both required */
    uint8_t        *flat_noise;         /* [n][lcus rounded up to a multiple of 64]   lcuFlatNoiseArray; 0 for LCUs the method never evaluates and in the tail */
    SvtAmdNoisePic *picture;            /* [n] */
} SvtAmdNoiseArrays;
SVT_AMD_API int svt_amd_noise_detect_batch_launch(SvtAmdContext *ctx, const SvtAmdNoiseJob *jobs, int num_jobs, const SvtAmdNoiseArrays *out);
#define SVT_AMD_NOISE_FLAT    0
#define SVT_AMD_NOISE_PICTURE 1
/* bytes ONE picture takes in array `which`; 0 for an unknown `which`.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_noise_detect_bytes(uint16_t luma_width, uint16_t luma_height, int which);

/*
 * Batched source-based operations: what SourceBasedOperationsKernel (Codec/EbSourceBasedOperationsProcess.c:1397) derives, per LCU and per picture, from the
 * records of the stages before it - and the two steps in front of it that feed it (EbHevcUpdateBeaInfoOverTime, DeriveSimilarCollocatedFlag) - for up to 256
 * pictures of ONE geometry per call, stream-ordered on the context's lane like svt_amd_picture_detect_batch_launch: the call never blocks and never copies to
 * the host.  Pure integer logic on records that already lie in HBM; no plane is read.  A batch of one picture is the single-picture form.
 * Job (all pointers DEVICE memory):
 *   stats           required: SvtAmdPaLcuStats[lcus] of the picture (svt_amd_side_stats_batch_launch)
 *   ref_stats       or NULL: the same array of the list-0 PA reference picture - the reference object's yMean[lcu] / variance[lcu] are that picture's 64x64
 *                   values (Codec/EbPictureAnalysisProcess.c:4323-4324).  NULL: both similarity flags are 0 (I pictures)
 *   chroma, detect, histogram   required: SvtAmdPaLcuChroma[lcus], SvtAmdPaLcuDetect[lcus] and the luma histogram [regions_w][regions_h][256] as
 *                   svt_amd_chroma_stats / picture_detect / side_stats _batch_launch left them
 *   zz[17], zz_count 0..17   SvtAmdZzLcu[lcus] of the picture itself (entry 0) and of the following pictures of the look-ahead window, in window order.  The window
 *                   is MIN(2 * period + 1, framesInSw, lookAheadDistance) pictures and ends in front of an I or end-of-sequence picture
 *                   (Codec/EbInitialRateControlProcess.c:534-553): that rule is the caller's, who passes fewer entries.  zz_count 0: no look-ahead, every
 *                   zz_cost / non_moving_index is 0xFF (EbHevcInitZzCostInfo, :573)
 *   me, ois         SvtAmdMeLcuResult[lcus] / SvtAmdOisLcuResult[lcus], or NULL: the records resident in picture slot cur_slot (the call waits, on the device,
 *                   for the launches that wrote them; the slot has to hold complete records of a picture of the batch's size; a later ME / OIS launch into
 *                   that slot from ANOTHER lane is the caller's to order behind this call, svt_amd_lane_event_record / _wait).  Read for P / B pictures and with
 *                   want_qpm only; an I picture without want_qpm ignores me, ois and cur_slot
 *   slice_type      0 I, 1 P, 2 B; temporal_layer_index 0..5; is_used_as_reference; resolution_class 0..3 (SequenceControlSet_t.inputResolution);
 *                   skip_ois_8x8, cu8x8_mode (PictureParentControlSet_t.skipOis8x8 / cu8x8Mode); want_qpm: improveSharpness || bitRateReduction ||
 *                   depthMode == PICT_LCU_SWITCH_DEPTH_MODE (:1585)
 * The rules, restated as the reference has them (nothing is repaired); "complete" is lcuParams->isCompleteLcu, unit validity lcuParams->rasterScanCuValidity
 * (Codec/EbSequenceControlSet.c:206, :277):
 *   zz_cost, non_moving_index   EbHevcUpdateBeaInfoOverTime (Codec/EbInitialRateControlProcess.c:519): the sum over the zz_count records / zz_count, (EB_U8).  Every
 *                   rule below reads these averaged values.
 *   similar_colocated(_all_layers)   DeriveSimilarCollocatedFlag (Codec/EbMotionEstimationProcess.c:462): |mean - refMean| < 10 and (|var * 100 / MAX(refVar, 1) -
 *                   100| < 10 or |var - refVar| < 10); similar_colocated only with is_used_as_reference.
 *   grass, skin, high_luma, high_chroma   GrassSkinLcu (:427): bit i is 16x16 unit i (raster), valid units only.  The 8x8 children carry their unit's flags
 *                   (:493-499), the 32x32 and 64x64 flags are the OR over their units (:501-517), so the masks carry everything.  In the reference the
 *                   parent flags are NEVER CLEARED: cuStatArray[parent] keeps a 1 for the life of the PCS pool object.  The device gives the per-picture value;
 *                   that stickiness lives in the caller's object (parent |= OR of the masks).  grass_percentage: GrassSkinPicture (:527).
 *   cmplx_contrast  SpatialHighContrastClassifier (:768), TemporalHighContrastClassifier (:741), PopulateFromCurrentLcuToNeighborLcus (:804).
 *                   lcuCmplxContrastArray is ORDER-DEPENDENT like isolated_high_intensity above: every LCU clears its own flag when the raster loop reaches it
 *                   (:1439) and a triggering LCU never marks itself, so the flag of n is 1 exactly when a triggering complete LCU m > n is one of n's eight
 *                   neighbours and the populate condition of that direction (:815-851) holds.
 *   dark_background_light_foreground, intra_coded_block_probability   LumaContrastDetectorLcu (:364) / Picture (:409): incomplete LCUs count in the moving /
 *                   non-moving means.
 *   failing_motion, uncovered_area   FailingMotionLcu (:169), DetectUncoveredLcu (:228): the (EB_S32) casts and the division (:211-212, :278-279) as written; the
 *                   OIS distortion is bits 0-19 of candidate[k][0].
 *   high_dark_area_density, high_dark_low_light_area_density, black_area_percentage   DeriveHighDarkAreaDensityFlag (:684): 32-bit sums and products as written.
 *   isolated_non_homogeneous   DetermineIsolatedNonHomogeneousRegionInPicture (:536): only the four diagonal neighbours are counted homogeneous (lcuVer != 0 &&
 *                   lcuHor != 0, :584); the flat-neighbour test is > 1 (:569).
 *   percentage_of_edge_in_light_background   DetermineMorePotentialAuraAreas (:639) with isEdgeLcu as Codec/EbSequenceControlSet.c:210 derives it.  A neighbour index
 *                   outside the picture's LCU array (the reference reads past it when a last-column LCU carries edge_block_num, which the detectors never set
 *                   there) counts as 0.
 *   complete_lcu_count, non_moving_index_average, zz_cost_average, low_motion_content   DerivePictureActivityStatistics (:81).  With no complete LCU the reference
 *                   leaves stale averages; the device writes 0 with complete_lcu_count 0.
 *   complex_lcu     DeriveBlockinessPresentFlag (:958) with IsSpatiallyComplexArea (:860), after the averages above: 0 / 1 / 2.  The neighbour tests compare signed:
 *                   in a picture below 64 samples a side the reference's unsigned forms (:922-939) read outside its arrays.
 *   cmplx_status    ComplexityClassifier32x32 (:120): 0 (CMPLX_LOW) / 4 (CMPLX_NOISE).
 *   intra_/inter_complexity_*, processed_leaf_count   with want_qpm: QpmGatherStatistics (:999) and the picture part (:1585-1660): the 8x8 units use their own OIS
 *                   distortion under cu8x8_mode 0 when its validDistortion bit (20) is set and fall back to the parent 16x16 (0 when that is not valid
 *                   either); depth 3 stays at its start values (min 0xFFFFFFFF, everything else 0) under skip_ois_8x8 (totDepths 3).  All zero without want_qpm.
 * Left to the host: CalculateAcEnergy (:302) exists as svt_amd_side_stats_batch_launch's ac_energy; SetDefaultDeltaQpRange (:609) is three table reads;
 * StationaryEdgeOverUpdateOverTimeLcu (:1142) walks the control sets of the look-ahead window.
 * Two stages in stream order: per LCU (a wave per LCU: a lane per 16x16 unit, a lane per 8x8 / 16x16 / 32x32 / 64x64 unit for the QPM statistics, lane shuffles),
 * the LCU's record and its partial sums stored - not added - into context-owned scratch; then a workgroup per picture that reduces the partials in LDS and runs
 * the passes that need the reduced values or the 3x3 neighbourhood.  The arrays are DEVICE memory, both required, picture i of the batch at i times
 * svt_amd_source_ops_bytes(...) bytes of each.  Everything is checked before anything is queued: a NULL required pointer, zz_count above 17 (or a NULL entry below
 * it), a layer above 5, a slice type above 2, a class above 3, a P / B picture or want_qpm whose ME / OIS records are neither given nor complete in a slot of the
 * batch's size, bad regions, a picture of more than 16384 LCUs or of more LCUs than the context was made for return SVT_AMD_ERR_BAD_PARAM
 * (svt_amd_last_error names the job) and queue nothing.
 */
typedef struct SvtAmdSboJob {
    const SvtAmdPaLcuStats   *stats;        /* required */
    const SvtAmdPaLcuStats   *ref_stats;    /* or NULL  */
    const SvtAmdPaLcuChroma  *chroma;       /* required */
    const SvtAmdPaLcuDetect  *detect;       /* required */
    const uint32_t           *histogram;    /* required: luma [regions_w][regions_h][256] */
    const SvtAmdZzLcu        *zz[17];       /* [0] the picture itself, then the window; entries from zz_count on are not read */
    const SvtAmdMeLcuResult  *me;           /* or NULL: cur_slot's */
    const SvtAmdOisLcuResult *ois;          /* or NULL: cur_slot's */
    int32_t cur_slot;
    uint8_t zz_count, slice_type, temporal_layer_index, is_used_as_reference;
    uint8_t resolution_class, skip_ois_8x8, cu8x8_mode, want_qpm;
    uint8_t pad[4];
} SvtAmdSboJob;                             /* 208 bytes */
typedef struct SvtAmdSboLcu {
    uint16_t grass, skin, high_luma, high_chroma; /* bit i: cuStatArray[RASTER_SCAN_TO_MD_SCAN[5 + i]].grassArea / skinArea / highLuma / highChroma (:480-491) */
    uint8_t  zz_cost, non_moving_index;     /* zzCostArray / nonMovingIndexArray after EbHevcUpdateBeaInfoOverTime                          */
    uint8_t  similar_colocated;             /* similarColocatedLcuArray                                                                     */
    uint8_t  similar_colocated_all_layers;  /* similarColocatedLcuArrayAllLayers                                                            */
    uint8_t  failing_motion;                /* failingMotionLcuFlag (:220, :1484)                                                           */
    uint8_t  uncovered_area;                /* uncoveredAreaLcuFlag (:292, :1494)                                                           */
    uint8_t  cmplx_contrast;                /* lcuCmplxContrastArray after the whole raster loop (:1439, :1514)                             */
    uint8_t  isolated_non_homogeneous;      /* lcuIsolatedNonHomogeneousAreaArray (:551, :597)                                              */
    uint8_t  cmplx_status;                  /* cmplxStatusLcu: 0 / 4 (:135, :160)                                                           */
    uint8_t  complex_lcu;                   /* complexLcuArray: 0 / 1 / 2 (:967-993)                                                        */
    uint8_t  pad[6];                        /* 0 */
} SvtAmdSboLcu;                             /* 24 bytes */
typedef struct SvtAmdSboPic {
    uint32_t complete_lcu_count;            /* completeLcuCount (:91)                     */
    uint32_t zz_cost_average;               /* zzCostAverage (:110)                       */
    uint16_t non_moving_index_average;      /* nonMovingIndexAverage (:109)               */
    uint8_t  low_motion_content;            /* lowMotionContentFlag (:112)                */
    uint8_t  dark_background_light_foreground; /* darkBackGroundlightForeGround (:416)    */
    uint8_t  intra_coded_block_probability; /* intraCodedBlockProbability (:420-423)      */
    uint8_t  grass_percentage;              /* grassPercentageInPicture (:530)            */
    uint8_t  percentage_of_edge_in_light_background; /* percentageOfEdgeinLightBackground (:677) */
    uint8_t  high_dark_area_density;        /* highDarkAreaDensityFlag (:704)             */
    uint8_t  high_dark_low_light_area_density; /* highDarkLowLightAreaDensityFlag (:726)  */
    uint8_t  black_area_percentage;         /* blackAreaPercentage (:724)                 */
    uint8_t  pad[6];                        /* 0 */
    uint32_t intra_complexity_min[4], intra_complexity_max[4], intra_complexity_accum[4], intra_complexity_avg[4]; /* by cuDepth (Codec/EbPictureControlSet.h:566-569) */
    uint32_t inter_complexity_min[4], inter_complexity_max[4], inter_complexity_accum[4], inter_complexity_avg[4]; /* (:570-573) */
    uint32_t processed_leaf_count[4];       /* processedleafCount (:574) */
} SvtAmdSboPic;                             /* 168 bytes */
typedef struct SvtAmdSboArrays {            /* DEVICE pointers, picture i of the batch at index i; both required */
    SvtAmdSboLcu *lcu;                      /* [n][lcus] */
    SvtAmdSboPic *picture;                  /* [n]       */
} SvtAmdSboArrays;
SVT_AMD_API int svt_amd_source_ops_batch_launch(SvtAmdContext *ctx, const SvtAmdSboJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                int regions_w, int regions_h, const SvtAmdSboArrays *out);
#define SVT_AMD_SBO_LCU     0
#define SVT_AMD_SBO_PICTURE 1
/* bytes ONE picture takes in array `which`; 0 for an unknown `which`.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_source_ops_bytes(uint16_t luma_width, uint16_t luma_height, int which);

/*
 * Batched mode-decision configuration: what ModeDecisionConfigurationKernel (Codec/EbModeDecisionConfigurationProcess.c:1905) with EarlyModeDecisionLcu
 * (Codec/EbModeDecisionConfiguration.c:1059) derives for a P or B picture from the records of the stages before it - the picture signals, the aura status,
 * the search method and the leaf list of every LCU (the lcu_md_mode, leaf_count, leaf_index and leaf_split fields of SvtAmdMdLcu) - for up to 256 pictures of
 * ONE geometry per call, stream-ordered on the context's lane like svt_amd_source_ops_batch_launch: the call never blocks and never copies to the host, and it
 * allocates at its first call only.  Pure integer logic on records that already lie in HBM; no plane is read.  A batch of one picture is the single-picture form.
 * Job (all pointers DEVICE memory, read where the earlier batches wrote them):
 *   me              SvtAmdMeLcuResult[lcus], or NULL: the records resident in picture slot cur_slot (the call waits, on the device, for the launches that
 *                   wrote them; the slot has to hold complete records of a picture of the batch's size; a later ME launch into that slot from ANOTHER lane
 *                   is the caller's to order behind this call, as for svt_amd_source_ops_batch_launch)
 *   stats, detect   required: svt_amd_side_stats_batch_launch's block statistics and svt_amd_picture_detect_batch_launch's LCU records
 *   sbo_lcu, sbo_pic   required: the two records of svt_amd_source_ops_batch_launch (want_qpm set: inter_complexity_min / max [0] are read)
 *   pic_detect, noise_pic   required: the picture records of svt_amd_picture_detect_batch_launch and svt_amd_noise_detect_batch_launch
 *   stationary_edge one byte per LCU (stationaryEdgeOverTimeFlag, the host's StationaryEdgeOverUpdateOverTimeLcu), or NULL - as the reference's NULL pointer:
 *                   the clause of IsAvcPartitioningMode that reads it never holds
 *   the scalars     the fields of the control sets the reference's host stages own, below.  slice_type is 1 (P) or 2 (B): the I-picture arm of DeriveLcuScore
 *                   (:1596) has no restatement pinned on the reference and is OUT OF SCOPE - an I picture is refused
 * The rules, restated as the reference has them (nothing is repaired; tests/mdc_numpy.py spells every width out):
 *   picture signals sceneCaracteristicId and adjustMinQPFlag (:1949-1975), highIntraSlection (:212-240), the chroma QP offsets (SetSliceAndPictureChromaQpOffsets :112),
 *                   tc / beta offset 0 (AdaptiveDlfParameterComputation :175), average_qp = the picture QP
 *   aura_status     AuraDetection / AuraDetection64x64 (:791-939): B pictures, LCUs with a column on either side and a row below; 128 (INVALID_AURA_STATUS)
 *                   everywhere else.  rightDist is assigned from topRDist (:888): the right neighbour's distortion is never read.  10 * cur and th * min are
 *                   32-bit products
 *   PICT_LCU_SWITCH pictures (depth_mode 0), DeriveLcuMdMode (:1826): ConfigureAdp (:1288), SetTargetBudgetOq (:1079), DeriveDefaultSegments (:942),
 *                   IsAvcPartitioningMode (:1232), ComputeRefinementCost, DeriveLcuScore (:1596; the score of a partial LCU is the wrapping mean over its
 *                   valid 8x8 units), PerformOutlierRemoval (:1736), DeriveOptimalBudgetPerLcu / SetLcuBudget (up to 101 passes), DeriveSearchMethod
 *                   (:1360-1392).  Every EB_U32 expression wraps at 32 bits; a score threshold of -1 multiplies as 0xFFFFFFFF (:1431); the deviation is the
 *                   SIGNED product ABS((EB_S32)(predictedCost - budget)) * 1000 (:1522), defined for pictures of up to 13,854 LCUs - larger ones are refused
 *   leaf list       PICT_LCU_SWITCH: Forward85 / 84 / 8x816x16 / 16x16CuToModeDecisionLCU (:370-704) for the full and AVC methods; EarlyModeDecisionLcu for the
 *                   open-loop methods - the 21 costs of depths 0..2 from the ME records (MdcInterCuRate :307; 64-bit), the 16 -> 32 and 32 -> 64 inter-depth
 *                   decisions with their running group counters (EbHevcMdcInterDepthDecision :715), EbHevcRefinementPredictionLoop (:436) with
 *                   EbHevcMdcRefinement (:82; the Pm3 arm tests Pm2, :232, as written), EbHevcForwardCuToModeDecision (:586); BDP and light-BDP LCUs:
 *                   leaf_count 0.  PICT_FULL85 / PICT_FULL84 pictures (1, 2): the two fixed lists.  Depth modes 3..5: leaf_count 0 - those pictures do not
 *                   go through the list.  Entries at and behind leaf_count are 0.
 * Left to the host: the scalars, StationaryEdgeOverUpdateOverTimeLcu (Codec/EbSourceBasedOperationsProcess.c:1142) and SetDefaultDeltaQpRange (:609).
 * Three stages in stream order - a wave per LCU (aura, AVC clause, score; stored - not added - into context-owned scratch), a workgroup per picture (the
 * budgeting loop, every LCU's score in LDS), a wave per LCU (the leaf list: a lane per coded unit, the 85-unit masks as wave ballots, the list a compaction in
 * MD-scan order).  No atomics, nothing to zero.  The arrays are DEVICE memory, both required, picture i of the batch at i times svt_amd_md_config_bytes(...)
 * bytes of each.  Everything is checked before anything is queued: a NULL required pointer or array, a slice type other than 1 / 2, a temporal layer or
 * hierarchical levels above 5, a class above 3, a depth mode above 5, a QP above 51, a picture of more than 13,854 LCUs or of more LCUs than the context was
 * made for, me == NULL with a slot that is out of range, holds no picture, one of another size or no complete ME records return SVT_AMD_ERR_BAD_PARAM
 * (svt_amd_last_error names the entry and the job), queue nothing and wait for nothing.
 */
#define SVT_AMD_MDC_MAX_LCUS 13854
typedef struct SvtAmdMdcJob {
    const SvtAmdMeLcuResult *me;            /* or NULL: cur_slot's; ppcs->meResults[lcu] (Codec/EbModeDecisionConfiguration.c:1015)           */
    const SvtAmdPaLcuStats  *stats;         /* required: ppcs->variance[lcu][0], ->yMean[lcu][0] (:1684, :1691)                              */
    const SvtAmdPaLcuDetect *detect;        /* required: sharpEdgeLcuFlag[lcu], edgeResultsPtr[lcu].edgeBlockNum (:1251, :1240)              */
    const SvtAmdSboLcu      *sbo_lcu;       /* required: similarColocatedLcuArrayAllLayers, complexLcuArray, failingMotionLcuFlag, nonMovingIndexArray */
    const SvtAmdSboPic      *sbo_pic;       /* required: grassPercentageInPicture, zzCostAverage, nonMovingIndexAverage, interComplexityMin / Max[0], ... */
    const SvtAmdPaPicDetect *pic_detect;    /* required: logoPicFlag (:1265)                                                                 */
    const SvtAmdNoisePic    *noise_pic;     /* required: picNoiseClass (:130, :1958, :1330)                                                  */
    const uint8_t           *stationary_edge; /* [lcus] or NULL: lcuStatArray[lcu].stationaryEdgeOverTimeFlag (:1242)                        */
    int32_t cur_slot;
    uint8_t slice_type;                     /* pcs->sliceType: 1 P, 2 B                                                                      */
    uint8_t temporal_layer_index;           /* pcs->temporalLayerIndex, 0..5                                                                 */
    uint8_t hierarchical_levels;            /* ppcs->hierarchicalLevels, 0..5                                                                */
    uint8_t is_used_as_reference;           /* ppcs->isUsedAsReferenceFlag                                                                   */
    uint8_t depth_mode;                     /* ppcs->depthMode - 1: 0 PICT_LCU_SWITCH, 1 FULL85, 2 FULL84, 3 BDP, 4 LIGHT_BDP, 5 OPEN_LOOP      */
    uint8_t enc_mode;                       /* pcs->encMode (SetTargetBudgetOq :1079)                                                        */
    uint8_t resolution_class;               /* scs->inputResolution, 0..3                                                                    */
    uint8_t qp;                             /* pcs->pictureQp, 0..51                                                                         */
    uint8_t is_pan, is_tilt;                /* ppcs->isPan, ->isTilt                                                                         */
    uint8_t noise_detection_th;             /* the noiseDetectionTh setting of svt_amd_noise_detect_batch_launch: class threshold 1 (0) or 3  */
    uint8_t homogeneity_percentage;         /* ppcs->picHomogenousOverTimeLcuPercentage (:1959)                                              */
    uint8_t frame_rate_30;                  /* (scs->staticConfig.frameRate >> 16) > 30 (:1684)                                              */
    uint8_t cu8x8_mode;                     /* ppcs->cu8x8Mode (Codec/EbModeDecisionConfiguration.c:474)                                     */
    uint8_t average_intensity;              /* ppcs->averageIntensity[0] (:1325)                                                             */
    uint8_t ref_average_intensity[2];       /* the list-0 / list-1 reference objects' averageIntensity                                       */
    uint8_t ref_intra_coded_area[2];        /* the reference objects' intraCodedArea and tmpLayerIdx: their test (:195) is overwritten ...   */
    uint8_t ref_temporal_layer[2];
    uint8_t ref_penalize_skip[2];           /* ... by the one of penalizeSkipflag (:221): only this pair is read                             */
    uint8_t pad;                            /* 0 */
    uint32_t lambda_sad;                    /* contextPtr->lambda: the SAD lambda of the picture's QP (Codec/EbModeDecisionConfiguration.c:1006) */
    uint32_t split_flag_bits[2];            /* mdRateEstimationPtr->splitFlagBits[0] and [3] (:1044-1045)                                    */
} SvtAmdMdcJob;                             /* 104 bytes */
typedef struct SvtAmdMdcLcu {
    uint8_t  leaf_count;                    /* the first 171 bytes: the head of SvtAmdMdLcu (MdcLcuData_t.leafCount, .leafDataArray[])        */
    uint8_t  leaf_index[SVT_AMD_ME_PU_COUNT], leaf_split[SVT_AMD_ME_PU_COUNT];
    uint8_t  lcu_md_mode;                   /* ppcs->lcuMdModeArray[lcu] (EB_LCU_DEPTH_MODE, Codec/EbDefinitions.h:1270); 0 unless PICT_LCU_SWITCH */
    uint8_t  aura_status;                   /* lcuPtr->auraStatus: 0, 1 or 128 (INVALID_AURA_STATUS)                                         */
    uint8_t  pred64;                        /* lcuPtr->pred64: EarlyModeDecisionLcu kept the 64x64 unit                                      */
    uint8_t  avc_partitioning;              /* IsAvcPartitioningMode (:1232); 0 unless PICT_LCU_SWITCH                                       */
    uint8_t  pad0;                          /* 0 */
    uint32_t lcu_score;                     /* lcuScoreArray[lcu] as the budgeting loop leaves it (:1420); 0 unless PICT_LCU_SWITCH           */
    uint8_t  lcu_cost;                      /* lcuCostArray[lcu]; 0 unless PICT_LCU_SWITCH                                                   */
    uint8_t  pad[3];                        /* 0 */
} SvtAmdMdcLcu;                             /* 184 bytes */
typedef struct SvtAmdMdcPic {
    uint8_t  scene_characteristic_id;       /* pcs->sceneCaracteristicId (:1949-1967)                                                        */
    uint8_t  adjust_min_qp;                 /* pcs->adjustMinQPFlag (:1969)                                                                  */
    uint8_t  high_intra_selection;          /* pcs->highIntraSlection (:212-240)                                                             */
    int8_t   slice_cb_qp_offset, slice_cr_qp_offset; /* SetSliceAndPictureChromaQpOffsets (:112)                                             */
    int8_t   tc_offset, beta_offset;        /* pcs->tcOffset, ->betaOffset: 0 (AdaptiveDlfParameterComputation :175-186)                     */
    uint8_t  average_qp;                    /* ppcs->averageQp (:2079)                                                                       */
    uint8_t  adp_depth_sensitive_picture_class; /* contextPtr->adpDepthSensitivePictureClass (ConfigureAdp :1288)                            */
    uint8_t  adp_refinement_mode;           /* contextPtr->adpRefinementMode (ComputeRefinementCost)                                         */
    uint8_t  number_of_segments;            /* contextPtr->numberOfSegments (DeriveDefaultSegments :942)                                     */
    uint8_t  pad0;                          /* 0 */
    uint32_t budget;                        /* contextPtr->budget (SetTargetBudgetOq :1079)                                                  */
    uint32_t predicted_cost;                /* contextPtr->predictedCost after the last pass                                                 */
    uint32_t lcu_min_score, lcu_max_score;  /* contextPtr->lcuMinScore, ->lcuMaxScore after PerformOutlierRemoval (:1736)                    */
    int8_t   score_th[7];                   /* contextPtr->scoreTh after the last pass                                                       */
    uint8_t  interval_cost[7];              /* contextPtr->intervalCost                                                                      */
    uint8_t  iterations;                    /* passes of the budgeting loop, 1..101                                                          */
    uint8_t  bdp_present, md_present;       /* pcs->bdpPresentFlag, ->mdPresentFlag (:1355-1390)                                             */
    uint8_t  pad[3];                        /* 0 */
} SvtAmdMdcPic;                             /* 48 bytes; everything from adp_depth_sensitive_picture_class on is 0 unless PICT_LCU_SWITCH */
typedef struct SvtAmdMdcArrays {            /* DEVICE pointers, picture i of the batch at index i; both required */
    SvtAmdMdcLcu *lcu;                      /* [n][lcus] */
    SvtAmdMdcPic *picture;                  /* [n]       */
} SvtAmdMdcArrays;
SVT_AMD_API int svt_amd_md_config_batch_launch(SvtAmdContext *ctx, const SvtAmdMdcJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                               const SvtAmdMdcArrays *out);
#define SVT_AMD_MDC_LCU     0
#define SVT_AMD_MDC_PICTURE 1
/* bytes ONE picture takes in array `which`; 0 for an unknown `which`.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_md_config_bytes(uint16_t luma_width, uint16_t luma_height, int which);
/* Development aid (tools/md_config_time.py): the stages the launches of this process run from now on - bit 0 k_mdc_lcu, bit 1 k_mdc_budget, bit 2 k_mdc_leaves;
 * 7 is the start value and the only one that gives complete records. */
SVT_AMD_API void svt_amd_debug_md_config_stages(int mask);

/*
 * Batched initial rate control: the look-ahead stage of InitialRateControlKernel (Codec/EbInitialRateControlProcess.c:849), the two per-LCU checks in front of it
 * in the ME process (StationaryEdgeOverUpdateOverTimeLcuPart1 / Part2, Codec/EbMotionEstimationProcess.c:502, :554) and the final stationary-edge stage of
 * SourceBasedOperationsKernel (StationaryEdgeOverUpdateOverTimeLcu, Codec/EbSourceBasedOperationsProcess.c:1142) - the stage the two blocks above leave to the
 * host - for up to 256 pictures of ONE geometry per call, stream-ordered on the context's lane like svt_amd_md_config_batch_launch: the call never blocks and
 * never copies to the host, and it allocates at its first call only.  Pure integer logic on records that already lie in HBM; no plane is read.  Its
 * stationary_edge array is what SvtAmdMdcJob.stationary_edge takes, its picture record holds SvtAmdMdcJob's is_pan, is_tilt and homogeneity_percentage.
 * Job (all pointers DEVICE memory):
 *   me              SvtAmdMeLcuResult[lcus], or NULL: the records resident in picture slot cur_slot - meaning, waits and refusals as for SvtAmdMdcJob.me.  Read
 *                   for P / B pictures and above temporal layer 0 (the only pictures whose rules read a vector or a distortion); an I picture of layer 0
 *                   ignores me and cur_slot
 *   stats           required: SvtAmdPaLcuStats[lcus] of the picture
 *   the three look-ahead lists, walked BY THE CALLER as SvtAmdSboJob.zz is - the queue rules (below) are the caller's, tests/irc_numpy.py window_lists spells
 *   them out.  Their entries may be arrays this same batch writes or arrays of earlier batches:
 *     edge_checks[4], edge_detect[4], edge_count 0..4   the SvtAmdIrcChecks and SvtAmdPaLcuDetect arrays of the window entries whose edges count
 *     hom_stats[16], hom_count 0..16                    the SvtAmdPaLcuStats arrays of the window entries the homogeneity sums run over
 *     pan_motion[8], pan_count 0..8                     the SvtAmdIrcMotion records of the non-I pictures among the first MIN(8, framesInSw) queue entries
 *   slice_type 0 I / 1 P / 2 B; temporal_layer_index <= hierarchical_levels <= 5; resolution_class 0..3; look_ahead: !endOfSequenceFlag && lookAheadDistance
 *   != 0; frames_to_check: noFramesToCheck = MIN(2 * predStructPeriod + 1, framesInSw, lookAheadDistance), 1..17 (1 without a look-ahead)
 * The rules, restated as the reference has them (nothing is repaired; tests/irc_numpy.py spells every width out).  "complete" is lcuParams->isCompleteLcu, "logo"
 * lcuParams->potentialLogoLcu (Codec/EbSequenceControlSet.c:216-273):
 *   check1, pm_check1   Part1 (:502), complete logo LCUs, 0 elsewhere: the four 32x32 variances (units 1..4), averageVar = sum >> 2, varOfVar = the int sum of
 *                   the four (EB_S32) squared differences, converted to EB_U64, >> 2 (:527-530); check1 = varOfVar > 50000 && lowMotion, pm_check1 = varOfVar >
 *                   1000; lowMotion: temporal layer 0, or |x| < 16 && |y| < 16 of meResults[lcu][0].xMvL0 / yMvL0 (EbHevcGetMv :431)
 *   check2, low_dist_logo   Part2 (:554), with look_ahead only: low_dist_logo = B picture && meResults[lcu][0].distortionDirection[0].distortion < 64 * 64 * (5
 *                   below class 2, else 2) on complete logo LCUs; check2 is assigned 1 unconditionally on the function's last line (:591) - 1 for EVERY LCU
 *                   with look_ahead, the 0 of the EB_MEMSET in EdgeDetectionMeanLumaChroma16x16 without
 *   motion          EbHevcDetectGlobalMotion (Codec/EbInitialRateControlProcess.c:218), P / B pictures, complete LCUs: the vector of the LCU against its left, top,
 *                   right and bottom neighbour - 0 / 0 at the left / top picture edge and where originX + 128 > width / originY + 128 > height; an
 *                   incomplete neighbour inside those bounds IS read - through CheckMvForPan, Tilt, PanHighAmp, TiltHighAmp (:30-116) with
 *                   GLOBAL_MOTION_THRESHOLD[hierarchicalLevels][temporalLayerIndex] (Codec/EbDefinitions.h:1184) and LOW_AMPLITUDE_TH 64; yCurrentMv < 64 is a
 *                   signed test, the products of two vectors are int.  is_pan_raw = totalPanLcus * 100 / totalCheckedLcus > 75, is_tilt_raw alike; no
 *                   complete LCU or an I picture: everything 0.  CheckForNonUniformMotionVectorField (:135) stores nothing and is not restated
 *   is_pan, is_tilt EbHevcUpdateGlobalMotionDetectionOverTime (:441) with look_ahead: over the first MIN(8, framesInSw) queue entries from the head - the picture
 *                   itself - I pictures skipped and not counted: is_pan = non-I picture && checked > 0 && pan * 100 / checked > 75 over the entries'
 *                   is_pan_raw; is_tilt is set to 0 and never set again; disableTmvpFlag never changes (its counter stays 0).  Without: the raw flags (:1020)
 *   similar_edge_count, pm_similar_edge_count   EbHevcUpdateMotionFieldUniformityOverTime (:598) with EbHevcStationaryEdgeCountLcu (:394): the walk covers
 *                   noFramesToCheck - 1 entries from the head (from index 0 when the head is the last queue index - not the start of
 *                   EbHevcUpdateBeaInfoOverTime), stops in front of an end-of-sequence picture, and only entries with (pictureNumber & 3) == 0 count: at most 4
 *                   of 16.  For an LCU with check1 && check2 (pm: pm_check1 && check2) every entry whose own check1 (pm_check1) is set adds its edge_cu bits
 *   var_of_var_over_time, homogeneous_over_time, homogeneity_percentage   UpdateHomogeneityOverTime (:646): the same walk, stopping in front of a scene-change
 *                   or end-of-sequence picture; the sums of the 64x64 variance and of its square - the int product of two promoted EB_U16, which does not
 *                   overflow for the variances of 8-bit pictures (below 16,384) - are divided by noFramesToCheck - 1, NOT by the entries walked (both 0 when
 *                   noFramesToCheck == 1); meanSqr - mean * mean in 64 bits, homogeneous: <= 4096; the percentage is (EB_U8)(count * 100 / lcuTotalCount).
 *                   Without look_ahead: 0xFFFFFFFFFFFFFFFF, 0 and 0 (ResetHomogeneityStructures :729)
 *   stationary_edge, pm_stationary_edge   StationaryEdgeOverUpdateOverTimeLcu with totalCheckedPictures = noFramesToCheck, with look_ahead only (0 without):
 *                   slideWindowTh = totalCheckedPictures / 4 - 1 is unsigned - below 4 pictures no flag is ever set; 1 where check1 && check2 (pm_check1 &&
 *                   check2) and at least 4 of the 16 counts exceed it; then three passes over the 3x3 window clamped at the picture edges: (a) a 1 whose
 *                   window holds no other 1 is cleared (the in-place raster loop equals this gather: tests/test_irc_cpu.py), (b) a 0 on a logo LCU with
 *                   check2 or incomplete becomes 2 next to a 1, (c) the same LCUs become 3 with more than three 2s in their window.  The PM plane uses the
 *                   same gate in (b) and (c): pm_check1 does not enter it (:1339, :1369)
 * Four stages in stream order - a wave per LCU (checks, votes; the workgroups' vote totals stored - not added - into context-owned scratch), a workgroup per
 * picture (the motion record), a wave per LCU behind the first stage of EVERY picture (a lane per 16x16 unit and flavour, the homogeneity sums a lane per
 * entry), a workgroup per picture (the passes with a byte per LCU in LDS, pan over time, the picture record).  No atomics, nothing to zero; every array is
 * written by one kernel only.  The arrays are DEVICE memory, all required, picture i of the batch at i times svt_amd_initial_rc_bytes(...) bytes of each.
 * Everything is checked before anything is queued: a NULL stats pointer or array, a count above its bound, a NULL entry below a count, a slice type above 2, a
 * layer above the levels, levels above 5, a class above 3, frames_to_check outside 1..17, look_ahead 0 with a non-empty list or frames_to_check other than 1, a
 * picture of more than 16,384 LCUs or of more LCUs than the context was made for, me == NULL (where it is read) with a slot that is out of range, holds no
 * picture, one of another size or no complete ME records return SVT_AMD_ERR_BAD_PARAM (svt_amd_last_error names the entry and the job), queue nothing and
 * wait for nothing.
 */
#define SVT_AMD_IRC_MAX_LCUS 16384
typedef struct SvtAmdIrcChecks {
    uint8_t check1;                         /* lcuStatArray[lcu].check1ForLogoStationaryEdgeOverTimeFlag (Codec/EbMotionEstimationProcess.c:532)   */
    uint8_t pm_check1;                      /* .pmCheck1ForLogoStationaryEdgeOverTimeFlag (:539)                                                  */
    uint8_t check2;                         /* .check2ForLogoStationaryEdgeOverTimeFlag (:591)                                                    */
    uint8_t low_dist_logo;                  /* .lowDistLogo (:578)                                                                                */
} SvtAmdIrcChecks;                          /* 4 bytes */
typedef struct SvtAmdIrcMotion {
    uint32_t total_checked_lcus, total_pan_lcus, total_tilt_lcus, total_pan_high_amp_lcus, total_tilt_high_amp_lcus; /* (Codec/EbInitialRateControlProcess.c:227-246) */
    uint8_t  is_pan_raw, is_tilt_raw;       /* ppcs->isPan, ->isTilt as EbHevcDetectGlobalMotion leaves them (:342-353)                           */
    uint8_t  pad[2];                        /* 0 */
} SvtAmdIrcMotion;                          /* 24 bytes */
typedef struct SvtAmdIrcLcu {
    uint8_t  similar_edge_count[16];        /* cuStatArray[RASTER_SCAN_CU_INDEX_16x16_0 + i].similarEdgeCount (:415)                              */
    uint8_t  pm_similar_edge_count[16];     /* .pmSimilarEdgeCount (:428)                                                                         */
    uint64_t var_of_var_over_time;          /* lcuVarianceOfVarianceOverTime[lcu] (:712)                                                          */
    uint8_t  homogeneous_over_time;         /* isLcuHomogeneousOverTime[lcu] (:714)                                                               */
    uint8_t  motion_votes;                  /* bit 0 pan, 1 tilt, 2 pan high amplitude, 3 tilt high amplitude (:298-338); 0: incomplete LCU, I picture */
    uint8_t  pad[6];                        /* 0 */
} SvtAmdIrcLcu;                             /* 48 bytes */
typedef struct SvtAmdIrcPic {
    uint8_t  is_pan, is_tilt;               /* ppcs->isPan, ->isTilt when the picture leaves the stage (:487-506, :1020)                          */
    uint8_t  homogeneity_percentage;        /* picHomogenousOverTimeLcuPercentage (:724)                                                          */
    uint8_t  pad0;                          /* 0 */
    uint16_t homogeneous_lcu_count;         /* countOfHomogeneousOverTime (:718)                                                                  */
    uint16_t stationary_lcu_count[4];       /* LCUs whose stationary_edge byte is 0, 1, 2, 3                                                      */
    uint8_t  pad[2];                        /* 0 */
} SvtAmdIrcPic;                             /* 16 bytes */
typedef struct SvtAmdIrcJob {
    const SvtAmdMeLcuResult *me;            /* or NULL: cur_slot's */
    const SvtAmdPaLcuStats  *stats;         /* required */
    const SvtAmdIrcChecks   *edge_checks[4]; /* entries from edge_count on are not read */
    const SvtAmdPaLcuDetect *edge_detect[4];
    const SvtAmdPaLcuStats  *hom_stats[16]; /* entries from hom_count on are not read */
    const SvtAmdIrcMotion   *pan_motion[8]; /* entries from pan_count on are not read */
    int32_t cur_slot;
    uint8_t edge_count, hom_count, pan_count;
    uint8_t slice_type, temporal_layer_index, hierarchical_levels, resolution_class;
    uint8_t look_ahead, frames_to_check;
    uint8_t pad[3];                         /* 0 */
} SvtAmdIrcJob;                             /* 288 bytes */
typedef struct SvtAmdIrcArrays {            /* DEVICE pointers, picture i of the batch at index i; all required */
    SvtAmdIrcChecks *checks;                /* [n][lcus] */
    SvtAmdIrcMotion *motion;                /* [n]       */
    SvtAmdIrcLcu    *lcu;                   /* [n][lcus] */
    uint8_t *stationary_edge;               /* [n][lcus rounded up to a multiple of 64]: stationaryEdgeOverTimeFlag, 0..3; the tail 0 */
    uint8_t *pm_stationary_edge;            /* the same of pmStationaryEdgeOverTimeFlag */
    SvtAmdIrcPic    *picture;               /* [n]       */
} SvtAmdIrcArrays;
SVT_AMD_API int svt_amd_initial_rc_batch_launch(SvtAmdContext *ctx, const SvtAmdIrcJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                const SvtAmdIrcArrays *out);
#define SVT_AMD_IRC_CHECKS        0
#define SVT_AMD_IRC_MOTION        1
#define SVT_AMD_IRC_LCU           2
#define SVT_AMD_IRC_STATIONARY    3
#define SVT_AMD_IRC_PM_STATIONARY 4
#define SVT_AMD_IRC_PICTURE       5
/* bytes ONE picture takes in array `which`; 0 for an unknown `which`.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_initial_rc_bytes(uint16_t luma_width, uint16_t luma_height, int which);

/*
 * Batched scene-transition detection: SceneTransitionDetector of the picture decision (Codec/EbPictureDecisionProcess.c:73-258) - the one function of that
 * process that reads data, and the one reader of the histograms svt_amd_side_stats_batch_launch and svt_amd_chroma_stats_batch_launch leave in HBM - for up to
 * 256 CONSECUTIVE CALLS of the detector per call of this entry, stream-ordered on the context's lane like svt_amd_initial_rc_batch_launch: the call never blocks
 * and never copies to the host, and it allocates at its first call only.  The host reads sizeof(SvtAmdScdPic) bytes a picture instead of 48 KB of histograms.
 * Job i is the detector's call for one picture: ParentPcsWindow[0] the past, [1] the current, [2] the future picture.  Job i starts from the state job i - 1
 * left (the running averages and resetRunningAvg of PictureDecisionContext_t); job 0 starts from *d_state_in (DEVICE), or from the constructor's state - all
 * averages 0, the flag 1 (:63-68) - when d_state_in is NULL.  state[n - 1] of one batch is the d_state_in of the next.  WHICH pictures get a call is the
 * caller's business, as the window lists of SvtAmdIrcJob are (PictureDecisionKernel :648-697): not picture 0, a past entry present, and four future entries
 * present with none of them at end of sequence.
 * Job (all pointers DEVICE memory, all required, read in place; they may be arrays an earlier launch on the same lane wrote):
 *   past_histogram, cur_histogram                 uint32_t[regions_w][regions_h][256]      SvtAmdSideArrays.histogram of the picture
 *   past_chroma_histogram, cur_chroma_histogram   uint32_t[regions_w][regions_h][2][256]   SvtAmdChromaArrays.histogram of the picture
 *   past_region_average, cur_region_average, future_region_average   the picture's 64-byte row of SvtAmdSideArrays.region_average; bytes 0 .. regions - 1 are read
 *   past_detect, cur_detect                       the SvtAmdPaPicDetect record, read for pic_avg_variance
 * Region (wi, hi) - wi the width index, the OUTER loop - is region wi * regions_h + hi of every [16] below.  The rules, restated as the reference has them
 * (nothing is repaired; tests/scd_numpy.py spells every width out, svt-hevc_amd/csrc/scd_logic.h is the one text the kernels compile), W x H the luma size:
 *   vote threshold  (EB_U32)((float)(regions * P) / 100 + 0.5), P 75 for scd_mode 2 and 50 otherwise (:126-128) = (regions * P + 50) / 100 in integers
 *   region size     regionWidth = W / regions_w and regionHeight = H / regions_h are set ONCE in front of the loops; inside them `regionWidth += W - regions_w *
 *                   regionWidth` runs in the last column and `regionHeight += H - regions_h * regionHeight` in the last row (:147-156), on the values the
 *                   iterations before left, in 32-bit unsigned arithmetic.  After k such steps a size is q + rem * (1 + (1 - regions) + .. + (1 - regions)^(k - 1))
 *                   with q the quotient and rem the remainder; the width has taken hi + 1 steps in the last column and none before it, the height wi + (hi ==
 *                   regions_h - 1).  With remainders of 0 (4 x 4 regions, sizes that are multiples of 8) every region is W / 4 x H / 4
 *   thresholds      T * ((regionWidth * regionHeight) >> 12) in 32 bits; T 4500 when |cur - past| of pic_avg_variance > 390 and either exceeds 1500, else 3000
 *                   (:158-163); for chroma a quarter of it
 *   ahd             per plane the sum over the 256 bins of |cur - past| (:167-172)
 *   running averages   with the reset flag all three take the three sums (:174-178); error = |average - ahd| per plane.  Only the luma average is updated
 *                   afterwards: the chroma averages change at a reset alone
 *   region class    abrupt: (error > th && ahd >= error) for luma, or the same with the chroma threshold for Cb or Cr; else gradual: error > th / 2 && ahd >=
 *                   error for luma (:185-194).  An abrupt region is a flash (class 2) when |future - past| < 5 && |future - cur| >= 5 && |cur - past| >= 5 of the
 *                   luma region averages, else a fade (3) when |future - cur| < 3 && |cur - past| < 3, else a scene change (4); its luma average is NOT
 *                   updated (:196-214).  A gradual region (1) and a region of neither class (0) set average = (3 * average + ahd) / 4 in 32 bits (:215-232)
 *   after the loops reset_running_avg = abrupt regions >= vote threshold; scene_change, the return value, = scene-change regions >= vote threshold (:243-256)
 * Two stages in stream order - a workgroup per region and job (a thread per bin, the three sums reduced by wave shuffles and four words of LDS, stored - not
 * added), then ONE wave with a lane per region that walks the jobs in order, its running averages in registers, the two counts population counts of wave
 * ballots.  No atomics, nothing to zero; every array is written by one kernel only.  The arrays are DEVICE memory, all required, job i at index i; every byte
 * of a job's part is written, pads and the entries of regions beyond regions_w * regions_h as 0.
 * regions_w, regions_h 1..4 each (MAX_NUMBER_OF_REGIONS_IN_WIDTH / _HEIGHT); scd_mode 1 or 2; luma_width, luma_height from 8 x 8 up to 16,384 LCUs - no picture
 * slot is read, so the picture need not fit the context.  Everything is checked before anything is queued: a NULL context, jobs or out, a job count outside
 * 1..256, regions outside 1..4, scd_mode outside 1..2, a size below 8 or above the bound, a NULL array or a NULL pointer in a job return SVT_AMD_ERR_BAD_PARAM
 * (svt_amd_last_error names the entry, and the job where one is at fault; a size above the bound is refused in the words all batched entries share, which say
 * "job 0" for the batch's size), queue nothing and wait for nothing.
 */
#define SVT_AMD_SCD_MAX_LCUS    16384
#define SVT_AMD_SCD_MAX_REGIONS 16
#define SVT_AMD_SCD_CLASS_NONE    0
#define SVT_AMD_SCD_CLASS_GRADUAL 1
#define SVT_AMD_SCD_CLASS_FLASH   2
#define SVT_AMD_SCD_CLASS_FADE    3
#define SVT_AMD_SCD_CLASS_SCENE   4
typedef struct SvtAmdScdJob {
    const uint32_t *past_histogram, *cur_histogram;
    const uint32_t *past_chroma_histogram, *cur_chroma_histogram;
    const uint8_t  *past_region_average, *cur_region_average, *future_region_average;
    const SvtAmdPaPicDetect *past_detect, *cur_detect;
} SvtAmdScdJob;                             /* 72 bytes */
typedef struct SvtAmdScdPic {
    uint8_t scene_change;                   /* the detector's return value: sceneChangeFlag (:697)                  */
    uint8_t reset_running_avg;              /* contextPtr->resetRunningAvg after the call (:243-248)                */
    uint8_t abrupt_regions;                 /* isAbruptChangeCount                                                  */
    uint8_t scene_regions;                  /* isSceneChangeCount                                                   */
    uint8_t region_count_threshold;         /* regionCountThreshold (:126-128)                                      */
    uint8_t pad[3];                         /* 0 */
    uint8_t region_class[16];               /* SVT_AMD_SCD_CLASS_*: the branch the region took; 0 beyond the regions */
} SvtAmdScdPic;                             /* 24 bytes */
typedef struct SvtAmdScdState {             /* PictureDecisionContext_t as the detector reads and leaves it */
    uint32_t ahd_running_avg[16];           /* ahdRunningAvg[wi][hi] at wi * regions_h + hi; written as 0 beyond the regions */
    uint32_t ahd_running_avg_cb[16];        /* ahdRunningAvgCb */
    uint32_t ahd_running_avg_cr[16];        /* ahdRunningAvgCr */
    uint8_t  reset_running_avg;             /* resetRunningAvg: any non-zero byte is a set flag; written as 0 / 1   */
    uint8_t  pad[3];                        /* 0 */
} SvtAmdScdState;                           /* 196 bytes */
typedef struct SvtAmdScdArrays {            /* DEVICE pointers, job i of the batch at index i; all required */
    SvtAmdScdPic   *picture;                /* [n]        */
    uint32_t       *ahd;                    /* [n][16][3]: the sums of luma, Cb, Cr per region */
    SvtAmdScdState *state;                  /* [n]: the context AFTER job i */
} SvtAmdScdArrays;
SVT_AMD_API int svt_amd_scene_detect_batch_launch(SvtAmdContext *ctx, const SvtAmdScdJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                  int regions_w, int regions_h, int scd_mode, const SvtAmdScdState *d_state_in, const SvtAmdScdArrays *out);
#define SVT_AMD_SCD_PICTURE 0
#define SVT_AMD_SCD_AHD     1
#define SVT_AMD_SCD_STATE   2
/* bytes ONE job takes in array `which`; 0 for an unknown `which` or regions outside 1..4.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_scene_detect_bytes(int which, int regions_w, int regions_h);
/* Development aid (tools/scd_time.py): the stages the launches of this process run from now on - bit 0 k_scd_ahd, bit 1 k_scd_decide; 3 is the start value and
 * the only one that gives complete results on arrays that hold none yet. */
SVT_AMD_API void svt_amd_debug_scene_detect_stages(int mask);

/*
 * Batched mode-decision LCU controls: the SvtAmdMdLcu records (below, "Device-resident mode decision") svt_amd_md_encode_picture* reads, assembled on the device from
 * the records of the batches above - what integration/svt_md_fill.h:svt_md_fill_lcu reads out of the reference's control sets on the host - for up to 256 pictures
 * of ONE geometry per call, stream-ordered on the context's lane like svt_amd_initial_rc_batch_launch: the call never blocks and never copies to the host, and it
 * allocates at its first call only.  svt_amd_md_picture_set_controls hands such an array to the mode-decision call, which reads it in place.
 * Job (all pointers DEVICE memory, read where the earlier batches wrote them):
 *   mdc_lcu         SvtAmdMdcLcu[lcus] of svt_amd_md_config_batch_launch, or NULL.  Its first 171 bytes are the head of SvtAmdMdLcu and are copied; lcu_md_mode
 *                   (kept under depth_mode 0 only, Codec/EbEncDecProcess.c:2893) and aura_status are read.  NULL is allowed with depth_mode 1 or 2 only
 *                   (PICT_FULL85 / PICT_FULL84): the fixed leaf list is built here as k_mdc_leaves builds it (Forward85 / 84CuToModeDecisionLCU,
 *                   Codec/EbModeDecisionConfiguration.c:370-484) and aura_status is 128 - the I pictures svt_amd_md_config_batch_launch refuses
 *   stats, detect, sbo_lcu, sbo_pic   required: the records of svt_amd_side_stats_ / picture_detect_ / source_ops_batch_launch
 *   irc_lcu, ac_energy   SvtAmdIrcLcu[lcus] of svt_amd_initial_rc_batch_launch and uint64_t[lcus][5] of svt_amd_side_stats_batch_launch: both, or both NULL -
 *                   then every contouring_class is 0
 *   stationary_edge uint8_t[lcus] of svt_amd_initial_rc_batch_launch, or NULL: all 0
 *   sticky          uint8_t[lcus], or NULL: bit 0 cuStatArray[0].highLuma, bit 1 cuStatArray[0].highChroma as the caller's pool object carried them from earlier
 *                   pictures (the note on cuStatArray[parent] in the source-ops block above); each is OR-ed with high_luma != 0 / high_chroma != 0
 *   slice_type 0 I / 1 P / 2 B (no rule reads it); depth_mode in SvtAmdMdcJob's encoding, 0..5; chroma_level 0..5; resolution_class 0..3; tile_cols x tile_rows
 *   uniformly spaced tiles, 1 .. the LCU columns / rows
 * The rules, restated as the reference has them (nothing is repaired; tests/mdctl_numpy.py spells them out):
 *   contouring_class[q]   DeriveContouringClass (Codec/EbModeDecisionConfiguration.c:395) of leaves 1, 22, 43, 64: 0 unless isLcuHomogeneousOverTime; on an edge LCU
 *                   (isEdgeLcu, Codec/EbSequenceControlSet.c:210: first column or row, or originX > width - 64, originY > height - 64) 2 / 3 / 3 below 1024 / 2048 /
 *                   3072 (ANTI_CONTOURING_TH_1, _2 and their unparenthesised sum), elsewhere 1 / 2 / 3 below 256 / 1024 / 2048; 64-bit comparisons of
 *                   lcuYSrcEnergyCuArray[lcu][1 + q]
 *   chroma_encode_mode   ConfigureChroma (Codec/EbModeDecisionProcess.c:383-437): cond0 stationary edge over time, cond1 homogeneous area && highChroma, cond2
 *                   !highLuma, cond3 grass_percentage > 60 || aura_status == 1 || is_pan; level 0 full, 1 best, 2 cond0 || 1 || 2, 3 cond0 || 1, 4 cond2 || 3,
 *                   5 cond0; 4:2:2 / 4:4:4 is always CHROMA_MODE_BEST (:435)
 *   tile_left / _top / _right   ConfigureLcuEdgeInfo (Codec/EbPictureControlSet.c:36) over tileColStartLcu[c] = c * columns / tile_cols (:743), rows alike
 *   the flags       as svt_md_fill_lcu: is_complete (EbSequenceControlSet.c:206), complexity_status_2, restrict_intra_global_motion ((is_pan || is_tilt) &&
 *                   non_moving_index < 2 && y_mean[0] < 50, Codec/EbEncDecProcess.c:2890), skip_small_cu (aura_status 0, no stationary edge), cmplx_noise
 *                   (cmplx_status == 4), variance_below_200, edge_block, no_stop_split (isolated_non_homogeneous, or aura_status 1 below class 3)
 * One stage - a wave per LCU: the head as words, a lane per byte of the tail, the record built in LDS and stored once as aligned words.  No atomics, nothing to
 * zero.  Every byte of SvtAmdMdLcu[n][lcus] is written (pads 0), none behind it.  Everything is checked before anything is queued: a NULL required pointer or
 * output array, mdc_lcu == NULL with a depth mode other than 1 / 2, exactly one of irc_lcu / ac_energy, a slice type above 2, a chroma level above 5, a class above
 * 3, a depth mode above 5, a tile count of 0 or above the LCU columns / rows, a non-zero pad, a picture of more than 16,384 LCUs or of more LCUs than the context
 * was made for, num_jobs outside 1..256 return SVT_AMD_ERR_BAD_PARAM (svt_amd_last_error names the entry and the job), queue nothing and wait for nothing.
 */
#define SVT_AMD_MDCTL_MAX_LCUS 16384
struct SvtAmdMdLcu;
typedef struct SvtAmdMdCtlJob {
    const SvtAmdMdcLcu      *mdc_lcu;       /* or NULL (depth_mode 1 / 2): pcs->mdcLcuArray[lcu] (integration/svt_md_fill.h:60), lcuPtr->auraStatus, ppcs->lcuMdModeArray */
    const SvtAmdPaLcuStats  *stats;         /* required: ppcs->variance[lcu][0], ->yMean[lcu][0] (Codec/EbCodingLoop.c:3866, EbEncDecProcess.c:2890)            */
    const SvtAmdPaLcuDetect *detect;        /* required: edgeResultsPtr[lcu].edgeBlockNum, lcuHomogeneousAreaArray[lcu] (Codec/EbModeDecisionProcess.c:389, :395) */
    const SvtAmdSboLcu      *sbo_lcu;       /* required: complexLcuArray, cmplxStatusLcu, lcuIsolatedNonHomogeneousAreaArray, nonMovingIndexArray, highLuma / highChroma */
    const SvtAmdSboPic      *sbo_pic;       /* required: grassPercentageInPicture (:397)                                                                        */
    const SvtAmdIrcLcu      *irc_lcu;       /* with ac_energy, or NULL: isLcuHomogeneousOverTime[lcu] (Codec/EbModeDecisionConfiguration.c:404)                 */
    const uint64_t          *ac_energy;     /* with irc_lcu, or NULL: [lcus][5] lcuYSrcEnergyCuArray[lcu][0..4] (:409-426)                                      */
    const uint8_t           *stationary_edge; /* [lcus] or NULL: lcuStatArray[lcu].stationaryEdgeOverTimeFlag (Codec/EbModeDecisionProcess.c:394)              */
    const uint8_t           *sticky;        /* [lcus] or NULL: bit 0 cuStatArray[0].highLuma, bit 1 .highChroma of the pool object (:395-396)                   */
    uint8_t slice_type;                     /* 0 I, 1 P, 2 B                                                                                                    */
    uint8_t depth_mode;                     /* ppcs->depthMode in the numbers of SvtAmdMdcJob.depth_mode: 0 PICT_LCU_SWITCH, 1 FULL85, 2 FULL84, ... 5 OPEN_LOOP   */
    uint8_t chroma_level;                   /* ModeDecisionContext_t.chromaLevel, 0..5 (:407-432)                                                               */
    uint8_t resolution_class;               /* scs->inputResolution, 0..3 (Codec/EbFullLoop.c:1445)                                                             */
    uint8_t is_pan, is_tilt;                /* ppcs->isPan, ->isTilt (SvtAmdIrcPic)                                                                             */
    uint8_t color_format_422_or_444;        /* pcs->colorFormat >= EB_YUV422 (:435)                                                                             */
    uint8_t pad0;                           /* 0 */
    uint16_t tile_cols, tile_rows;          /* ppcs->tileColumnCount, ->tileRowCount (Codec/EbPictureControlSet.c:743-746)                                      */
    uint8_t pad[4];                         /* 0 */
} SvtAmdMdCtlJob;                           /* 88 bytes */
SVT_AMD_API int svt_amd_md_controls_batch_launch(SvtAmdContext *ctx, const SvtAmdMdCtlJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                 struct SvtAmdMdLcu *out);
#define SVT_AMD_MDCTL_LCU 0
/* bytes ONE picture takes in array `which`; 0 for an unknown `which`.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_md_controls_bytes(uint16_t luma_width, uint16_t luma_height, int which);
/* What the mode-decision call learns about a bound device array (svt_amd_md_picture_set_controls) without reading it on the host: one record per picture */
typedef struct SvtAmdMdCtlCheck {
    uint32_t bad_leaf_count;                /* LCUs whose leaf_count is outside 1..85                                          */
    uint32_t bad_leaf_list;                 /* LCUs whose leaf list (its first MIN(leaf_count, 85) entries) is not strictly ascending or holds an index above 84 */
    uint32_t md_mode[16];                   /* LCUs by lcu_md_mode; values above 15 count in bin 15                            */
    uint32_t bad_chroma;                    /* LCUs whose chroma_encode_mode is neither 1 nor 2                                */
    uint32_t tiles;                         /* LCUs with tile_left && tile_top                                                 */
    uint32_t first_bad;                     /* the first LCU the call refuses, 0xFFFFFFFF: none                                */
    uint32_t first_kind;                    /* of that LCU: 0 leaf_count, 1 leaf list, 2 not decided by ModeDecisionLcu (P / B calls only) */
} SvtAmdMdCtlCheck;                         /* 88 bytes */
/* debug / test: that record of n DEVICE records under SvtAmdMdPicture.depth_mode, for an I (inter 0) or a P / B call; blocking */
SVT_AMD_API int svt_amd_debug_md_controls_check(SvtAmdContext *ctx, const struct SvtAmdMdLcu *d_lcus, int n, int depth_mode, int inter, SvtAmdMdCtlCheck *out);


/* Device-side timing of the launches issued between begin/end on the context's
 * own stream (HIP events); used for roofline.achieved in bench.py. */
SVT_AMD_API int svt_amd_timer_begin(SvtAmdContext *ctx);
SVT_AMD_API int svt_amd_timer_end(SvtAmdContext *ctx, float *elapsed_ms);
/* Average duration (ms) and launch count of the named kernel class since the
 * last svt_amd_timer_begin; kernel_class in {"me_search","me_subpel","prep"} */
SVT_AMD_API int svt_amd_kernel_time(SvtAmdContext *ctx, const char *kernel_class,
                                    float *avg_ms, int *launches);

/* Development aid: per-workgroup phase clock stamps of the next batched ME launch
 * (call with out == NULL to arm for `workgroups` = jobs x max LCUs, again with a buffer of
 * workgroups*16 u64 to collect).  tools/me_phase_profile.py prints the breakdown. */
SVT_AMD_API int svt_amd_debug_me_phase_profile(SvtAmdContext *ctx, size_t workgroups,
                                               unsigned long long *out);

/* Debug/parity access to the device-built planes of a slot (host copies).
 * which: 0 full, 1 quarter, 2 sixteenth, 3 half-pel b, 4 half-pel h, 5 half-pel j.
 * Copies the whole padded allocation; out_stride / out_pad describe it. */
SVT_AMD_API int svt_amd_picture_read_plane(SvtAmdContext *ctx, int slot, int which, uint8_t *dst,
                                           size_t dst_capacity, uint32_t *out_stride,
                                           uint32_t *out_pad, uint32_t *out_rows);

/* ------------------------------------------------------------------------- */
/* LEAF layer (table-slot replacements; host pointers; synchronous)          */
/* Each comment names the reference typedef/table and the C_DEFAULT symbol.  */
/* ------------------------------------------------------------------------- */

/* EB_SADKERNELNxM_TYPE, NxMSadKernel_funcPtrArray (EbComputeSAD.h:95);
 * C peer FastLoop_NxMSadKernel (C_DEFAULT/EbComputeSAD_C.c:147). */
SVT_AMD_API uint32_t svt_amd_NxMSadKernel(const uint8_t *src, uint32_t srcStride,
                                          const uint8_t *ref, uint32_t refStride,
                                          uint32_t height, uint32_t width);

/* EB_SADLOOPKERNELNxM_TYPE, NxMSadLoopKernel_funcPtrArray (EbComputeSAD.h:152);
 * C peer SadLoopKernel (C_DEFAULT/EbComputeSAD_C.c:170). */
SVT_AMD_API void svt_amd_SadLoopKernel(const uint8_t *src, uint32_t srcStride,
                                       const uint8_t *ref, uint32_t refStride,
                                       uint32_t height, uint32_t width, uint64_t *bestSad,
                                       int16_t *xSearchCenter, int16_t *ySearchCenter,
                                       uint32_t srcStrideRaw, int16_t searchAreaWidth,
                                       int16_t searchAreaHeight);

/* EB_SADAVGKERNELNxM_TYPE, NxMSadAveragingKernel_funcPtrArray (EbComputeSAD.h:123);
 * C peer CombinedAveragingSAD (C_DEFAULT/EbComputeSAD_C.c:14). */
SVT_AMD_API uint32_t svt_amd_NxMSadAveragingKernel(const uint8_t *src, uint32_t srcStride,
                                                   const uint8_t *ref1, uint32_t ref1Stride,
                                                   const uint8_t *ref2, uint32_t ref2Stride,
                                                   uint32_t height, uint32_t width);

/* GetEightHorizontalSearchPointResults_8x8_16x16_funcPtrArray (EbComputeSAD.h);
 * C peer GetEightHorizontalSearchPointResults_8x8_16x16_PU (EbComputeSAD_C.c:252). */
SVT_AMD_API void svt_amd_GetEightHorizontalSearchPointResults_8x8_16x16_PU(
    const uint8_t *src, uint32_t srcStride, const uint8_t *ref, uint32_t refStride,
    uint32_t *pBestSad8x8, uint32_t *pBestMV8x8, uint32_t *pBestSad16x16,
    uint32_t *pBestMV16x16, uint32_t mv, uint16_t *pSad16x16);

/* GetEightHorizontalSearchPointResults_32x32_64x64_funcPtrArray;
 * C peer GetEightHorizontalSearchPointResults_32x32_64x64 (EbComputeSAD_C.c:372). */
SVT_AMD_API void svt_amd_GetEightHorizontalSearchPointResults_32x32_64x64(
    const uint16_t *pSad16x16, uint32_t *pBestSad32x32, uint32_t *pBestSad64x64,
    uint32_t *pBestMV32x32, uint32_t *pBestMV64x64, uint32_t mv);

/* SadCalculation_8x8_16x16_funcPtrArray (EbMeSadCalculation.h:106);
 * C peer SadCalculation_8x8_16x16 (C_DEFAULT/EbMeSadCalculation_C.c:14). */
SVT_AMD_API void svt_amd_SadCalculation_8x8_16x16(
    const uint8_t *src, uint32_t srcStride, const uint8_t *ref, uint32_t refStride,
    uint32_t *pBestSad8x8, uint32_t *pBestSad16x16, uint32_t *pBestMV8x8,
    uint32_t *pBestMV16x16, uint32_t mv, uint32_t *pSad16x16);

/* SadCalculation_32x32_64x64_funcPtrArray; C peer EbMeSadCalculation_C.c:64. */
SVT_AMD_API void svt_amd_SadCalculation_32x32_64x64(
    const uint32_t *pSad16x16, uint32_t *pBestSad32x32, uint32_t *pBestSad64x64,
    uint32_t *pBestMV32x32, uint32_t *pBestMV64x64, uint32_t mv);

/* AvcStyleUniPredLumaIFFunctionPtrArray[..][1|2] (EbAvcStyleMcp.h:111);
 * C peers AvcStyleLumaInterpolationFilterHorizontal/Vertical (EbAvcStyleMcp_C.c:34,62). */
SVT_AMD_API void svt_amd_AvcStyleLumaInterpolationFilterHorizontal(
    const uint8_t *refPic, uint32_t srcStride, uint8_t *dst, uint32_t dstStride,
    uint32_t puWidth, uint32_t puHeight, uint8_t *tempBuf, uint32_t fracPos);
SVT_AMD_API void svt_amd_AvcStyleLumaInterpolationFilterVertical(
    const uint8_t *refPic, uint32_t srcStride, uint8_t *dst, uint32_t dstStride,
    uint32_t puWidth, uint32_t puHeight, uint8_t *tempBuf, uint32_t fracPos);

/* PictureAverageArray (EbAvcStyleMcp.h:129); C peer PictureAverageKernel
 * (C_DEFAULT/EbPictureOperators_C.c:46). */
SVT_AMD_API void svt_amd_PictureAverageKernel(const uint8_t *src0, uint32_t src0Stride,
                                              const uint8_t *src1, uint32_t src1Stride,
                                              uint8_t *dst, uint32_t dstStride,
                                              uint32_t areaWidth, uint32_t areaHeight);

/* SpatialFullDistortionKernel_funcPtrArray (EbPictureOperators.h:633);
 * C peer SpatialFullDistortionKernel (C_DEFAULT/EbPictureOperators_C.c:643). */
SVT_AMD_API uint64_t svt_amd_SpatialFullDistortionKernel(const uint8_t *input, uint32_t inputStride,
                                                         const uint8_t *recon, uint32_t reconStride,
                                                         uint32_t areaWidth, uint32_t areaHeight);

/* Decimation2D (EbPictureAnalysisProcess.c:173) - not table-dispatched in the
 * reference but the producer of the HME inputs. */
SVT_AMD_API void svt_amd_Decimation2D(const uint8_t *inputSamples, uint32_t inputStride,
                                      uint32_t inputAreaWidth, uint32_t inputAreaHeight,
                                      uint8_t *decimSamples, uint32_t decimStride,
                                      uint32_t decimStep);

/* ------------------------------------------------------------------------- */
/* EncDec leaf families: residual, transforms, quantisation, distortion, SATD */
/* ------------------------------------------------------------------------- */

/* BATCHED forms (device pointers; block b of a size x size batch at base + b*size*size).
 * kind: 0 DCT, 1 low-precision "Estimate" DCT (32/16 only), 2 DST (4x4 only).
 * Replace the per-TU calls EstimateTransform/EncodeTransform -> Transform* (EbTransforms.c:3268,3343;
 * tables EbTransforms.h:339-510), EstimateInvTransform/EncodeInvTransform (:3455,3502),
 * QuantizeInvQuantize via UnifiedQuantizeInvQuantize (EbTransforms.c:2978), PictureFullDistortionLuma
 * -> FullDistortionKernel*_32bit (EbPictureOperators.c:397; table EbPictureOperators.h:503) and
 * Compute8x8Satd/Compute4x4Satd (EbPictureOperators.c:186-262, EbHmCode.c:41). */
SVT_AMD_API int svt_amd_fwd_transform_batch(SvtAmdContext *ctx, int kind, int size, uint32_t bitIncrement,
                                            const int16_t *d_residual, int16_t *d_coeff, uint32_t nblocks);
SVT_AMD_API int svt_amd_inv_transform_batch(SvtAmdContext *ctx, int kind, int size, uint32_t bitIncrement,
                                            const int16_t *d_coeff, int16_t *d_residual, uint32_t nblocks);
/* The 32x32 transforms as integer-MFMA products (v_mfma_i32_32x32x32_i8; txfm_mfma.hip): same results as the two calls above for
 * size 32 (kind 0 DCT / 1 "Estimate" DCT forward; inverse DCT), every int16 input - blocks of the Estimate form whose 16-bit
 * butterfly levels would wrap (C_DEFAULT/EbTransforms_C.c:492-520; impossible for 8-bit residuals) are redone by the VALU kernel. */
SVT_AMD_API int svt_amd_fwd_transform_mfma_batch(SvtAmdContext *ctx, int kind, int size, uint32_t bitIncrement,
                                                 const int16_t *d_residual, int16_t *d_coeff, uint32_t nblocks);
SVT_AMD_API int svt_amd_inv_transform_mfma_batch(SvtAmdContext *ctx, int size, uint32_t bitIncrement, const int16_t *d_coeff,
                                                 int16_t *d_residual, uint32_t nblocks);
SVT_AMD_API int svt_amd_quantize_batch(SvtAmdContext *ctx, int size, uint32_t qFunc, uint32_t q_offset,
                                       int32_t shiftedQBits, int32_t shiftedFFunc, int32_t iq_offset,
                                       int32_t shiftNum, const int16_t *d_coeff, int16_t *d_quant,
                                       int16_t *d_recon, uint32_t *d_nz, uint32_t nblocks);
/* mode: 0 FullDistortionKernel_32bit, 1 ...CbfZero_32bit, 2 ...Intra_32bit; d_result = 2 x u64 per block */
SVT_AMD_API int svt_amd_full_distortion_batch(SvtAmdContext *ctx, int size, int mode, const int16_t *d_coeff,
                                              const int16_t *d_recon, uint64_t *d_result, uint32_t nblocks);
SVT_AMD_API int svt_amd_satd_batch(SvtAmdContext *ctx, int size, const int16_t *d_diff, uint64_t *d_satd,
                                   uint32_t nblocks);

/* LEAF forms: EB_TRANS_COEFF_* tables (EbTransforms.h:339-510); C peers C_DEFAULT/EbTransforms_C.c:1602-2119 */
#define SVT_AMD_DECL_TRANSFORM(name)                                                                      \
    SVT_AMD_API void svt_amd_##name(int16_t *src, const uint32_t srcStride, int16_t *dst,                 \
                                    const uint32_t dstStride, int16_t *transformInnerArrayPtr,            \
                                    uint32_t bitIncrement);
SVT_AMD_DECL_TRANSFORM(Transform32x32)
SVT_AMD_DECL_TRANSFORM(Transform32x32Estimate)
SVT_AMD_DECL_TRANSFORM(Transform16x16)
SVT_AMD_DECL_TRANSFORM(Transform16x16Estimate)
SVT_AMD_DECL_TRANSFORM(Transform8x8)
SVT_AMD_DECL_TRANSFORM(Transform4x4)
SVT_AMD_DECL_TRANSFORM(DstTransform4x4)
SVT_AMD_DECL_TRANSFORM(InvTransform32x32)
SVT_AMD_DECL_TRANSFORM(InvTransform16x16)
SVT_AMD_DECL_TRANSFORM(InvTransform8x8)
SVT_AMD_DECL_TRANSFORM(InvTransform4x4)
SVT_AMD_DECL_TRANSFORM(InvDstTransform4x4)

/* QiQ_funcPtrArray (EbTransforms.h:271-296); C peer QuantizeInvQuantize (EbTransforms_C.c:89) */
SVT_AMD_API void svt_amd_QuantizeInvQuantize(int16_t *coeff, const uint32_t coeffStride, int16_t *quantCoeff,
                                             int16_t *reconCoeff, const uint32_t qFunc, const uint32_t q_offset,
                                             const int32_t shiftedQBits, const int32_t shiftedFFunc,
                                             const int32_t iq_offset, const int32_t shiftNum,
                                             const uint32_t areaSize, uint32_t *nonzerocoeff);
/* FullDistortionIntrinsic_funcPtrArray (EbPictureOperators.h:503); C peers EbPictureOperators_C.c:385-480 */
SVT_AMD_API void svt_amd_FullDistortionKernel_32bit(int16_t *coeff, uint32_t coeffStride, int16_t *reconCoeff,
                                                    uint32_t reconCoeffStride, uint64_t distortionResult[2],
                                                    uint32_t areaWidth, uint32_t areaHeight);
SVT_AMD_API void svt_amd_FullDistortionKernelCbfZero_32bit(int16_t *coeff, uint32_t coeffStride, int16_t *reconCoeff,
                                                           uint32_t reconCoeffStride, uint64_t distortionResult[2],
                                                           uint32_t areaWidth, uint32_t areaHeight);
SVT_AMD_API void svt_amd_FullDistortionKernelIntra_32bit(int16_t *coeff, uint32_t coeffStride, int16_t *reconCoeff,
                                                         uint32_t reconCoeffStride, uint64_t distortionResult[2],
                                                         uint32_t areaWidth, uint32_t areaHeight);
/* Compute8x8Satd_funcPtrArray (EbPictureOperators.h); C peers EbPictureOperators_C.c:481,563, EbHmCode.c:41,127 */
SVT_AMD_API uint64_t svt_amd_Compute8x8Satd(int16_t *diff);
SVT_AMD_API uint64_t svt_amd_Compute4x4Satd(int16_t *diff);
SVT_AMD_API uint64_t svt_amd_Compute8x8Satd_U8(uint8_t *src, uint64_t *dcValue, uint32_t srcStride);
SVT_AMD_API uint64_t svt_amd_Compute4x4Satd_U8(uint8_t *src, uint64_t *dcValue, uint32_t srcStride);
/* ResidualKernel_funcPtrArray / AdditionKernel_funcPtrArray (EbPictureOperators.h:242-330);
 * C peers ResidualKernel (:297), PictureAdditionKernel (:112) */
SVT_AMD_API void svt_amd_ResidualKernel(uint8_t *input, uint32_t inputStride, uint8_t *pred, uint32_t predStride,
                                        int16_t *residual, uint32_t residualStride, uint32_t areaWidth,
                                        uint32_t areaHeight);
SVT_AMD_API void svt_amd_PictureAdditionKernel(uint8_t *predPtr, uint32_t predStride, int16_t *residualPtr,
                                               uint32_t residualStride, uint8_t *reconPtr, uint32_t reconStride,
                                               uint32_t width, uint32_t height);

/* ------------------------------------------------------------------------- */
/* Intra prediction kernels                                                   */
/* ------------------------------------------------------------------------- */
/* mode ids of the batched form, in the order of the reference's kernel tables
 * (Codec/EbIntraPrediction.h:470-648) */
enum SvtAmdIntraKernel {
    SVT_AMD_INTRA_VERTICAL_LUMA = 0, SVT_AMD_INTRA_VERTICAL_CHROMA, SVT_AMD_INTRA_HORIZONTAL_LUMA,
    SVT_AMD_INTRA_HORIZONTAL_CHROMA, SVT_AMD_INTRA_DC_LUMA, SVT_AMD_INTRA_DC_CHROMA, SVT_AMD_INTRA_PLANAR,
    SVT_AMD_INTRA_ANGULAR_34, SVT_AMD_INTRA_ANGULAR_18, SVT_AMD_INTRA_ANGULAR_2,
    SVT_AMD_INTRA_ANGULAR_VERTICAL, SVT_AMD_INTRA_ANGULAR_HORIZONTAL
};
/* block b: reference samples at d_refs + b*ref_pitch (samples; layout [0..2N) left, [2N] top-left,
 * [2N+1..4N] top; refSampMain = block base + main_offset for the two generic angular kernels),
 * prediction written to d_pred + b*size*size (stride = size). */
SVT_AMD_API int svt_amd_intra_pred_batch(SvtAmdContext *ctx, int mode, int bytes_per_sample, int size, int skip,
                                         int32_t intraPredAngle, const void *d_refs, uint32_t ref_pitch,
                                         int32_t main_offset, void *d_pred, uint32_t nblocks);

/* LEAF forms: EB_INTRA_NOANG_TYPE / EB_INTRA_NOANG_16bit_TYPE / EB_INTRA_ANG_TYPE (EbIntraPrediction.h:430-466);
 * C peers C_DEFAULT/EbIntraPrediction_C.c:15-1051 */
#define SVT_AMD_DECL_INTRA(name, T)                                                                        \
    SVT_AMD_API void svt_amd_##name(const uint32_t size, T *refSamples, T *predictionPtr,                  \
                                    const uint32_t predictionBufferStride, const uint8_t skip);
#define SVT_AMD_DECL_INTRA_ANG(name, T)                                                                    \
    SVT_AMD_API void svt_amd_##name(uint32_t size, T *refSampMain, T *predictionPtr,                       \
                                    uint32_t predictionBufferStride, const uint8_t skip, int32_t intraPredAngle);
SVT_AMD_DECL_INTRA(IntraModeVerticalLuma, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeVerticalLuma16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeVerticalChroma, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeVerticalChroma16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeHorizontalLuma, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeHorizontalLuma16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeHorizontalChroma, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeHorizontalChroma16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeDCLuma, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeDCLuma16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeDCChroma, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeDCChroma16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModePlanar, uint8_t)
SVT_AMD_DECL_INTRA(IntraModePlanar16bit, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeAngular_34, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeAngular16bit_34, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeAngular_18, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeAngular16bit_18, uint16_t)
SVT_AMD_DECL_INTRA(IntraModeAngular_2, uint8_t)
SVT_AMD_DECL_INTRA(IntraModeAngular16bit_2, uint16_t)
SVT_AMD_DECL_INTRA_ANG(IntraModeAngular_Vertical_Kernel, uint8_t)
SVT_AMD_DECL_INTRA_ANG(IntraModeAngular16bit_Vertical_Kernel, uint16_t)
SVT_AMD_DECL_INTRA_ANG(IntraModeAngular_Horizontal_Kernel, uint8_t)
SVT_AMD_DECL_INTRA_ANG(IntraModeAngular16bit_Horizontal_Kernel, uint16_t)

/* ------------------------------------------------------------------------- */
/* In-loop filters (deblocking, SAO) and 10-bit pack/unpack                   */
/* ------------------------------------------------------------------------- */
/* One 4-sample luma edge: `offset` = sample index of q0 of the first edge sample inside the plane;
 * tc/beta as derived by the reference's LCU drivers (EbDeblockingFilter.c:2222-3600, tables :33-66). */
typedef struct SvtAmdDlfLumaEdge { int32_t offset; int16_t tc, beta; uint8_t vertical, pad[3]; } SvtAmdDlfLumaEdge;
typedef struct SvtAmdDlfChromaEdge { int32_t offset; uint8_t cb_tc, cr_tc, vertical, pad; } SvtAmdDlfChromaEdge;
/* per-LCU SAO statistics, the four output arrays of GatherSaoStatisticsLcu* in one record */
typedef struct SvtAmdSaoStats {
    int32_t boDiff[32]; uint16_t boCount[32]; int32_t eoDiff[4][5]; uint16_t eoCount[4][5];
} SvtAmdSaoStats;

/* BATCHED (device pointers).  Edges of one launch must not overlap. */
SVT_AMD_API int svt_amd_dlf_luma_edges_batch(SvtAmdContext *ctx, void *d_plane, uint32_t stride,
                                             int bytes_per_sample, const SvtAmdDlfLumaEdge *d_edges, uint32_t nedges);
SVT_AMD_API int svt_amd_dlf_chroma_edges_batch(SvtAmdContext *ctx, void *d_cb, void *d_cr, uint32_t stride,
                                               int bytes_per_sample, const SvtAmdDlfChromaEdge *d_edges,
                                               uint32_t nedges);
/* WHOLE PICTURE boundary-strength derivation (device pointers): replaces the per-coding-unit calls SetBSArrayBasedOnPUBoundary
 * (Codec/EbDeblockingFilter.c:339) and SetBSArrayBasedOnTUBoundary (:472) with CalculateBSForPUBoundary (:109) that the
 * encode pass makes against its neighbour arrays (EbCodingLoop.c:3546-4450).  d_map: one entry per 8x8 block, raster
 * (mode: 1 INTER_MODE / 2 INTRA_MODE of the covering coding unit, dir: its interPredDirectionIndex, size_log2: log2 of the
 * coding-unit size, mv: predictionUnitArray[0].mv); d_cbf = pictureControlSetPtr->cbfMapArray (luma cbf per 4x4 block,
 * row pitch width / 4); ref_poc0 / 1 = refPOC of the two reference lists; d_lcu_edge: per LCU, 1 = tile left edge, 2 = tile
 * top edge.  Output = the layout svt_amd_dlf_picture reads ([lcu raster][256]). */
typedef struct SvtAmdCuMapEntry { uint8_t mode, dir, size_log2, pad; int16_t mv[2][2]; } SvtAmdCuMapEntry;
SVT_AMD_API int svt_amd_bs_picture(SvtAmdContext *ctx, const SvtAmdCuMapEntry *d_map, const uint8_t *d_cbf, uint32_t width,
                                   uint32_t height, int slice_type, uint64_t ref_poc0, uint64_t ref_poc1,
                                   const uint8_t *d_lcu_edge, uint8_t *d_bs_v, uint8_t *d_bs_h);
/* WHOLE PICTURE (device pointers, 4:2:0, in place): the state the per-LCU drivers LCUInternalAreaDLFCore /
 * LCUBoundaryDLFCore / LCUPictureEdgeDLFCore (+16bit; Codec/EbDeblockingFilter.c:2222, 2828, 3518, called per LCU from
 * EbCodingLoop.c:4600-4631) leave once every LCU has been through them.  d_y/d_cb/d_cr point at sample (0,0) of the
 * planes (strides in samples); d_bs_v / d_bs_h = pictureControlSetPtr->verticalEdgeBSArray / horizontalEdgeBSArray laid
 * out [lcu raster][256] (index = 4x4 block raster inside the 64x64 LCU, EbDeblockingFilter.h:19-22); d_qp = qpArray
 * (one byte per 8x8 block, row pitch qpStride); offsets = the picture control set's tcOffset / betaOffset / cbQpOffset /
 * crQpOffset.  width and height are multiples of 8.  Tile and picture boundaries carry strength 0 in the arrays. */
SVT_AMD_API int svt_amd_dlf_picture(SvtAmdContext *ctx, int bytes_per_sample, void *d_y, uint32_t strideY, void *d_cb,
                                    void *d_cr, uint32_t strideC, uint32_t width, uint32_t height,
                                    const uint8_t *d_bs_v, const uint8_t *d_bs_h, const uint8_t *d_qp, uint32_t qpStride,
                                    int32_t tcOffset, int32_t betaOffset, int32_t cbQpOffset, int32_t crQpOffset);
/* WHOLE PICTURE SAO application (device pointers, 4:2:0, OUT OF PLACE: d_dst[k] != d_src[k]): replaces
 * ApplySaoOffsetsPicture(16bit) -> ApplySaoOffsetsLcu(16bit) (Codec/EbEncDecProcess.c:522-757, :215-517; 16-bit :762-1330).
 * One record per LCU (raster order): SaoParameters_t (Codec/EbCodingUnit.h:137-146; type[0] luma, type[1] chroma:
 * 0 off, 1..4 edge offset 0 / 90 / 135 / 45 degrees, 5 band offset) with the two merge flags squeezed into bytes and the
 * tile-edge flags of lcuEdgeInfoPtr / tileInfoPtr that ApplySaoOffsetsLcu reads (:252-256) in edge_flags.
 * luma_on / chroma_on = pictureControlSetPtr->saoFlag[0] / [1]. */
typedef struct SvtAmdSaoLcuParams {
    uint8_t  merge_left, merge_up;
    uint8_t  edge_flags;        /* 1 tile left edge, 2 tile right edge, 4 tile top edge, 8 tile bottom edge */
    uint8_t  pad;
    uint32_t type[2];
    int32_t  offset[3][4];
    uint32_t band[3];
} SvtAmdSaoLcuParams;
SVT_AMD_API int svt_amd_sao_apply_picture(SvtAmdContext *ctx, int bytes_per_sample, const void *const d_src[3],
                                          void *const d_dst[3], uint32_t strideY, uint32_t strideC, uint32_t width,
                                          uint32_t height, const SvtAmdSaoLcuParams *d_lcus, int luma_on, int chroma_on);
/* SAO parameter decision of a whole picture from per-LCU statistics (device pointers): replaces the part of
 * SaoGenerationDecision / SaoGenerationDecision16bit after the statistics gathering (Codec/
 * EbSampleAdaptiveOffsetGenerationDecision.c:647-850, :936-1140): DetermineSaoLumaModeOffsets (:44), DetermineSaoChroma
 * ModeOffsets (:182), the reduced luma mode of temporal layers 0 / 1 (:347) and TestSaoCopyModes (:437).  Every LCU's own
 * best parameters are independent; the merge test needs the final parameters of the left and the upper LCU and runs as a
 * wavefront over anti-diagonals.  d_stats_y / cb / cr: [lcu raster] records as svt_amd_sao_gather_picture writes them;
 * d_enable: per LCU (NULL = all 1), 0 = the encode pass's shut-off conditions hold (EbCodingLoop.c:4675-4697), parameters
 * become zero; 1 = decide; 2 = d_params already holds this LCU's final parameters (an earlier call), a merge candidate only;
 * d_params: in: edge_flags (1 / 4 = no left / upper merge candidate), out: everything else; d_costs: [lcu][2] the luma and
 * chroma best costs the reference's call returns (also the work space between the two passes). */
typedef struct SvtAmdSaoDecisionParams {
    uint64_t lambda, chroma_lambda;                 /* contextPtr->fullLambda / fullChromaLambdaSao                      */
    uint32_t type_bits[6], merge_bits[2], offset_bits[8]; /* mdRateEstimationPtr->saoTypeIndexBits / MergeFlagBits / OffsetTrunUnaryBits */
    uint8_t  is_10bit, mm_sao, temporal_layer, pad; /* mm_sao = contextPtr->saoMode                                      */
} SvtAmdSaoDecisionParams;
SVT_AMD_API int svt_amd_sao_decide_picture(SvtAmdContext *ctx, const SvtAmdSaoDecisionParams *params, const SvtAmdSaoStats *d_stats_y,
                                           const SvtAmdSaoStats *d_stats_cb, const SvtAmdSaoStats *d_stats_cr, uint32_t lcu_cols,
                                           uint32_t lcu_rows, const uint8_t *d_enable, SvtAmdSaoLcuParams *d_params,
                                           int64_t *d_costs);
/* ONE LCU (host pointers, synchronous): the same decision with the neighbours' final parameters handed in (NULL = no
 * candidate), i.e. exactly the inputs SaoGenerationDecision has once its statistics are gathered. */
SVT_AMD_API int svt_amd_sao_decide_lcu(SvtAmdContext *ctx, const SvtAmdSaoDecisionParams *params, const SvtAmdSaoStats *stats_y,
                                       const SvtAmdSaoStats *stats_cb, const SvtAmdSaoStats *stats_cr,
                                       const SvtAmdSaoLcuParams *left, const SvtAmdSaoLcuParams *up, SvtAmdSaoLcuParams *out,
                                       int64_t costs[2]);
/* statistics of every LCU of a plane (raster LCU order), replaces the per-LCU SaoGenerationDecision ->
 * GatherSaoStatisticsLcu* calls (EbSampleAdaptiveOffsetGenerationDecision.c:647,936) */
SVT_AMD_API int svt_amd_sao_gather_picture(SvtAmdContext *ctx, int bytes_per_sample, const void *d_input,
                                           uint32_t inputStride, const void *d_recon, uint32_t reconStride,
                                           uint32_t width, uint32_t height, uint32_t lcu_size,
                                           int only_eo_90_45_135, SvtAmdSaoStats *d_stats);
/* plane-level 8+2 bit -> 16 bit pack (compressed = 4 two-bit samples per byte) and the inverse */
SVT_AMD_API int svt_amd_pack_plane(SvtAmdContext *ctx, const uint8_t *d_in8, uint32_t in8Stride, const uint8_t *d_inn,
                                   uint32_t innStride, int compressed, uint16_t *d_out16, uint32_t outStride,
                                   uint32_t width, uint32_t height);
SVT_AMD_API int svt_amd_unpack_plane(SvtAmdContext *ctx, const uint16_t *d_in16, uint32_t inStride, uint8_t *d_out8,
                                     uint32_t out8Stride, uint8_t *d_outn, uint32_t outnStride, uint32_t width,
                                     uint32_t height);

/* LEAF forms.  Luma4SampleEdgeDLFCore_Table / Chroma2SampleEdgeDLFCore_Table (EbDeblockingFilter.h:245-272) */
SVT_AMD_API void svt_amd_Luma4SampleEdgeDLFCore(uint8_t *edgeStartFilteredSamplePtr, uint32_t reconLumaPicStride,
                                                uint8_t isVerticalEdge, int32_t tc, int32_t beta);
SVT_AMD_API void svt_amd_Luma4SampleEdgeDLFCore16bit(uint16_t *edgeStartFilteredSamplePtr, uint32_t reconLumaPicStride,
                                                     uint8_t isVerticalEdge, int32_t tc, int32_t beta);
SVT_AMD_API void svt_amd_Chroma2SampleEdgeDLFCore(uint8_t *edgeStartSampleCb, uint8_t *edgeStartSampleCr,
                                                  uint32_t reconChromaPicStride, uint8_t isVerticalEdge, uint8_t cbTc,
                                                  uint8_t crTc);
SVT_AMD_API void svt_amd_Chroma2SampleEdgeDLFCore16bit(uint16_t *edgeStartSampleCb, uint16_t *edgeStartSampleCr,
                                                       uint32_t reconChromaPicStride, uint8_t isVerticalEdge,
                                                       uint8_t cbTc, uint8_t crTc);
/* SaoGatherFunctionTable* (EbSampleAdaptiveOffset.h:171-206); return EB_ERRORTYPE (0 = EB_ErrorNone) */
SVT_AMD_API int svt_amd_GatherSaoStatisticsLcuLossy_62x62(uint8_t *inputSamplePtr, uint32_t inputStride,
                                                          uint8_t *reconSamplePtr, uint32_t reconStride, uint32_t lcuWidth,
                                                          uint32_t lcuHeight, int32_t *boDiff, uint16_t *boCount,
                                                          int32_t eoDiff[4][5], uint16_t eoCount[4][5]);
SVT_AMD_API int svt_amd_GatherSaoStatisticsLcu_62x62_16bit(uint16_t *inputSamplePtr, uint32_t inputStride,
                                                           uint16_t *reconSamplePtr, uint32_t reconStride, uint32_t lcuWidth,
                                                           uint32_t lcuHeight, int32_t *boDiff, uint16_t *boCount,
                                                           int32_t eoDiff[4][5], uint16_t eoCount[4][5]);
SVT_AMD_API int svt_amd_GatherSaoStatisticsLcu_OnlyEo_90_45_135_Lossy(uint8_t *inputSamplePtr, uint32_t inputStride,
                                                                      uint8_t *reconSamplePtr, uint32_t reconStride,
                                                                      uint32_t lcuWidth, uint32_t lcuHeight,
                                                                      int32_t eoDiff[4][5], uint16_t eoCount[4][5]);
SVT_AMD_API int svt_amd_GatherSaoStatisticsLcu_62x62_OnlyEo_90_45_135_16bit(uint16_t *inputSamplePtr, uint32_t inputStride,
                                                                            uint16_t *reconSamplePtr, uint32_t reconStride,
                                                                            uint32_t lcuWidth, uint32_t lcuHeight,
                                                                            int32_t eoDiff[4][5], uint16_t eoCount[4][5]);
/* SaoFunctionTableEO_* / BO tables (EbSampleAdaptiveOffset.h:209-360) */
SVT_AMD_API int svt_amd_SAOApplyBO(uint8_t *reconSamplePtr, uint32_t reconStride, uint32_t saoBandPosition,
                                   int8_t *saoOffsetPtr, uint32_t lcuHeight, uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_0(uint8_t *reconSamplePtr, uint32_t reconStride, uint8_t *temporalBufferLeft,
                                     int8_t *saoOffsetPtr, uint32_t lcuHeight, uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_90(uint8_t *reconSamplePtr, uint32_t reconStride, uint8_t *temporalBufferUpper,
                                      int8_t *saoOffsetPtr, uint32_t lcuHeight, uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_135(uint8_t *reconSamplePtr, uint32_t reconStride, uint8_t *temporalBufferLeft,
                                       uint8_t *temporalBufferUpper, int8_t *saoOffsetPtr, uint32_t lcuHeight,
                                       uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_45(uint8_t *reconSamplePtr, uint32_t reconStride, uint8_t *temporalBufferLeft,
                                      uint8_t *temporalBufferUpper, int8_t *saoOffsetPtr, uint32_t lcuHeight,
                                      uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyBO16bit(uint16_t *reconSamplePtr, uint32_t reconStride, uint32_t saoBandPosition,
                                        int8_t *saoOffsetPtr, uint32_t lcuHeight, uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_0_16bit(uint16_t *reconSamplePtr, uint32_t reconStride, uint16_t *temporalBufferLeft,
                                           int8_t *saoOffsetPtr, uint32_t lcuHeight, uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_90_16bit(uint16_t *reconSamplePtr, uint32_t reconStride, uint16_t *temporalBufferUpper,
                                            int8_t *saoOffsetPtr, uint32_t lcuHeight, uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_135_16bit(uint16_t *reconSamplePtr, uint32_t reconStride, uint16_t *temporalBufferLeft,
                                             uint16_t *temporalBufferUpper, int8_t *saoOffsetPtr, uint32_t lcuHeight,
                                             uint32_t lcuWidth);
SVT_AMD_API int svt_amd_SAOApplyEO_45_16bit(uint16_t *reconSamplePtr, uint32_t reconStride, uint16_t *temporalBufferLeft,
                                            uint16_t *temporalBufferUpper, int8_t *saoOffsetPtr, uint32_t lcuHeight,
                                            uint32_t lcuWidth);
/* Pack2D_funcPtrArray_16Bit_SRC ... UnPackAvg_funcPtrArray (EbPackUnPack.h:27-175) */
SVT_AMD_API void svt_amd_EB_ENC_msbPack2D(uint8_t *in8BitBuffer, uint32_t in8Stride, uint8_t *innBitBuffer,
                                          uint16_t *out16BitBuffer, uint32_t innStride, uint32_t outStride,
                                          uint32_t width, uint32_t height);
SVT_AMD_API void svt_amd_CompressedPackmsb(uint8_t *in8BitBuffer, uint32_t in8Stride, uint8_t *innBitBuffer,
                                           uint16_t *out16BitBuffer, uint32_t innStride, uint32_t outStride,
                                           uint32_t width, uint32_t height);
SVT_AMD_API void svt_amd_CPack_C(const uint8_t *innBitBuffer, uint32_t innStride, uint8_t *inCompnBitBuffer,
                                 uint32_t outStride, uint8_t *localCache, uint32_t width, uint32_t height);
SVT_AMD_API void svt_amd_EB_ENC_msbUnPack2D(uint16_t *in16BitBuffer, uint32_t inStride, uint8_t *out8BitBuffer,
                                            uint8_t *outnBitBuffer, uint32_t out8Stride, uint32_t outnStride,
                                            uint32_t width, uint32_t height);
SVT_AMD_API void svt_amd_UnPack8BitData(uint16_t *in16BitBuffer, uint32_t inStride, uint8_t *out8BitBuffer,
                                        uint32_t out8Stride, uint32_t width, uint32_t height);
SVT_AMD_API void svt_amd_UnpackAvg(uint16_t *ref16L0, uint32_t refL0Stride, uint16_t *ref16L1, uint32_t refL1Stride,
                                   uint8_t *dstPtr, uint32_t dstStride, uint32_t width, uint32_t height);

/* ------------------------------------------------------------------------- */
/* Coefficient rate estimation (mode-decision full loop / encode pass)        */
/* ------------------------------------------------------------------------- */
/* Same layout as the reference's CabacCost_t (Codec/EbCabacContextModel.h:216-226), filled on the host by
 * PrecomputeCabacCost (Codec/EbCoeffEstimation_Intrinsic.c:161) from the CABAC context state. */
typedef struct SvtAmdCabacCost {
    uint32_t CabacBitsLast[60 * 2 + 28 * 2];
    uint8_t  CabacBitsSig[2 * 42];
    uint8_t  CabacBitsG1[2 * 24];
    uint8_t  CabacBitsG2[2 * 6];
    uint8_t  CabacBitsSigMl[2 * 4];
    uint16_t CabacBitsG1x[24 / 4 * 16];
    uint8_t  CabacBitsSigV[32][16];
} SvtAmdCabacCost;
/* per-TU side information of the batched form */
typedef struct SvtAmdTuInfo {
    uint32_t num_nonzero;      /* numNonZeroCoeffs: the true count of non-zero coefficients (0 -> 0 bits) */
    uint8_t  type;             /* INTER_MODE 1 / INTRA_MODE 2 (Codec/EbDefinitions.h:345)                 */
    uint8_t  intra_luma_mode, intra_chroma_mode, component; /* component: 0 luma, else chroma            */
} SvtAmdTuInfo;
/* BATCHED: bits of nblocks contiguous size x size blocks (block b at d_coeff + b*size*size); d_bits[b] = the amount
 * EstimateQuantizedCoefficients_Lossy (EbCoeffEstimation_Intrinsic.c:1415) adds to *coeffBitsLong for that TU.
 * `cost` is a HOST pointer (copied to the device by the call). */
SVT_AMD_API int svt_amd_coeff_bits_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, uint32_t size,
                                         const int16_t *d_coeff, const SvtAmdTuInfo *d_info, uint64_t *d_bits,
                                         uint32_t nblocks);
/* The CABAC-context-UPDATING estimator: EstimateQuantizedCoefficients_generic_Update / _Update_SSE2 (Codec/EbEntropyCoding.c:2986,
 * 9355; table EstimateQuantizedCoefficientsUpdate, EbEntropyCoding.h:387), used by the mode decision's full loops when
 * coeffCabacUpdate is on (EbEncDecProcess.c:2115-2123).  Context models are SVT_AMD_COEFF_CTX_WORDS 32-bit words in
 * CoeffCtxtMdl_t's order (EbCabacContextModel.h:204-214): lastSigX[30] lastSigY[30] sig[42] coeffGroupSig[4] greater1[24]
 * greater2[6]; every call leaves the updated states in place.
 * BATCHED: nblocks contiguous size x size blocks; consecutive runs of chain_len blocks share model d_ctx_models[run] and are
 * walked in order (the units of one candidate).  d_bits[b] = the amount added to *coeffBitsLong (15 fractional bits). */
#define SVT_AMD_COEFF_CTX_WORDS 136
SVT_AMD_API int svt_amd_coeff_bits_update_batch(SvtAmdContext *ctx, uint32_t size, const int16_t *d_coeff, const SvtAmdTuInfo *d_info,
                                                uint32_t *d_ctx_models, uint64_t *d_bits, uint32_t nblocks, uint32_t chain_len);
/* LEAF, reference signature (CoeffCtxtMdl_t * as uint32_t *) */
SVT_AMD_API int svt_amd_EstimateQuantizedCoefficients_Update(uint32_t *updatedCoeffCtxModel, SvtAmdCabacCost *CabacCost, void *cabacEncodeCtxPtr,
                                                             uint32_t size, uint32_t type, uint32_t intraLumaMode, uint32_t intraChromaMode,
                                                             int16_t *coeffBufferPtr, const uint32_t coeffStride, uint32_t componentType,
                                                             uint32_t numNonZeroCoeffs, uint64_t *coeffBitsLong);
/* LEAF: slot [1][*] of EstimateQuantizedCoefficients (Codec/EbEntropyCoding.h:334-347); cabacEncodeCtxPtr unused, as in
 * the reference; returns EB_ERRORTYPE (0 = EB_ErrorNone). */
SVT_AMD_API int svt_amd_EstimateQuantizedCoefficients_Lossy(SvtAmdCabacCost *CabacCost, void *cabacEncodeCtxPtr,
                                                            uint32_t size, uint32_t type, uint32_t intraLumaMode,
                                                            uint32_t intraChromaMode, int16_t *coeffBufferPtr,
                                                            const uint32_t coeffStride, uint32_t componentType,
                                                            uint32_t numNonZeroCoeffs, uint64_t *coeffBitsLong);

/* ------------------------------------------------------------------------- */
/* Luma full loop of one mode-decision candidate                              */
/* ------------------------------------------------------------------------- */
/* Replaces ProductFullLoop (Codec/EbFullLoop.c:185-446; caller PerformFullLoop, EbProductCodingLoop.c:4351-4460) for
 * the configuration the presets >= encMode 5 use: no RDOQ / PM-core, coefficient-domain distortion, no CABAC-context
 * update (Codec/EbEncDecProcess.c:2028-2205).  Per transform unit: EstimateTransform (EbTransforms.c:3268) ->
 * ProductUnifiedQuantizeInvQuantizeMd (EbFullLoop.c:77) -> PictureFullDistortionLuma (EbPictureOperators.c:397) ->
 * TuEstimateCoeffBitsLuma (EbEntropyCoding.c:7899) -> TuCalcCostLuma (EbRateDistortionCost.c:289).  A 64x64 CU is four
 * 32x32 transform units (TU index 1..4), smaller CUs one (TU index 0). */
typedef struct SvtAmdFullLoopIn {
    uint32_t size;              /* CU size 8 / 16 / 32 / 64                                              */
    uint32_t qp;
    uint32_t slice_type;        /* EB_PICTURE: 0 B, 1 P, 2 I, 3 IDR (selects the quantiser dead zone)    */
    uint16_t pf_mode;           /* contextPtr->pfMdMode: 0 off, 1 N2, 2 N4                               */
    uint16_t pm_core;           /* contextPtr->rdoqPmCoreMethod: 0 EB_NO_RDOQ, 2 EB_PMCORE (encMode 1..4: every 4x4 block
                                 * of levels re-decided among 100 / 70 / 50 % scalings, EbTransforms.c:2807-2950)      */
    uint32_t cand_type;         /* INTER_MODE 1 / INTRA_MODE 2                                           */
    uint32_t intra_luma_mode;
    uint32_t full_lambda;       /* contextPtr->fullLambda                                                */
    uint32_t cbf_bits[4];       /* mdRateEstimationPtr->lumaCbfBits[0], [1], [5], [6]                    */
    uint32_t ycbf;              /* candidatePtr->yCbf before the call                                    */
    uint64_t coeff_bits;        /* *yCoeffBits before the call (accumulated)                             */
    uint64_t dist[2];           /* yFullDistortion before the call (accumulated for 64x64)               */
} SvtAmdFullLoopIn;
typedef struct SvtAmdFullLoopOut {
    uint32_t nz[5];             /* yCountNonZeroCoeffs[0..4] entries this call wrote (others 0)          */
    uint32_t ycbf;              /* candidatePtr->yCbf after the call                                     */
    uint64_t coeff_bits;        /* *yCoeffBits after the call                                            */
    uint64_t dist[2];           /* yFullDistortion[DIST_CALC_RESIDUAL / PREDICTION] after the call       */
    int16_t  ydc[4];            /* candidateBuffer->yDc                                                  */
    uint16_t cand_nz[4];        /* candidateBuffer->yCountNonZeroCoeffs                                  */
} SvtAmdFullLoopOut;
/* BATCHED: candidate c has its size x size luma residual at d_residual + c*4096 (row pitch = size); the quantised
 * and the reconstructed coefficients are written in the same layout.  `cost` is a HOST pointer. */
SVT_AMD_API int svt_amd_full_loop_luma_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost,
                                             const SvtAmdFullLoopIn *d_in, const int16_t *d_residual,
                                             int16_t *d_quant, int16_t *d_recon, SvtAmdFullLoopOut *d_out,
                                             uint32_t ncand);
/* Same arguments; serves the candidates whose pm_core is EB_PMCORE (2) and leaves the others alone, as the call above leaves
 * those alone: ProductUnifiedQuantizeInvQuantizeMd -> DecoupledQuantizeInvQuantizeLoops (Codec/EbFullLoop.c:121-148,
 * EbTransforms.c:2605-2973) - a picture-level switch of encMode 1..4 (EbEncDecProcess.c:2201). */
SVT_AMD_API int svt_amd_full_loop_luma_pmcore_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost,
                                                    const SvtAmdFullLoopIn *d_in, const int16_t *d_residual,
                                                    int16_t *d_quant, int16_t *d_recon, SvtAmdFullLoopOut *d_out,
                                                    uint32_t ncand);
/* Per-call form on HOST pointers (row pitch `pitch` samples, e.g. the reference's 64-sample LCU buffers); writes back
 * only the (T >> pf) area of every transform unit, like the reference.  Blocking; used by the ProductFullLoop binding. */
SVT_AMD_API int svt_amd_full_loop_luma(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdFullLoopIn *in,
                                       const int16_t *residual, int16_t *quant, int16_t *recon, uint32_t pitch,
                                       SvtAmdFullLoopOut *out);

/* ------------------------------------------------------------------------- */
/* Distortion stage of the mode decision's fast loop                           */
/* ------------------------------------------------------------------------- */
/* Replaces, for a list of candidates whose predictions are already on the device (svt_amd_intra_pu_batch /
 * svt_amd_inter_pu_batch), the measurement ProductPerformFastLoop makes after ProductMdFastPuPrediction (Codec/
 * EbProductCodingLoop.c:2036-2078): luma SAD of the predicted block against the source block (NxMSadKernel_funcPtrArray,
 * C_DEFAULT/EbComputeSAD_C.c:147) and, with contextPtr->useChromaInformationInFastLoop, Cb SAD + Cr SAD; most-probable-mode
 * candidates skip it.  What stays with the caller: the candidate that reuses its open-loop distortion (:2042-2043), the
 * ">> 2" of zero-motion 64x64 candidates in noise LCUs (:2079-2090) and the fast-cost functions themselves (scalar).
 * 8-bit 4:2:0; offsets and strides in samples; the chroma planes may be NULL when no candidate sets flag 1. */
typedef struct SvtAmdFastLoopCand {
    int32_t src_off_y, src_off_c;      /* the coding unit's block inside the source planes                         */
    int32_t pred_off_y, pred_off_c;    /* the candidate's block inside the prediction planes                       */
    uint8_t size;                      /* 8 / 16 / 32 / 64                                                         */
    uint8_t flags;                     /* 1: with chroma (useChromaInformationInFastLoop); 2: mpmFlag, skip        */
    uint8_t pad[2];
} SvtAmdFastLoopCand;
typedef struct SvtAmdFastLoopDist { uint32_t luma, chroma; } SvtAmdFastLoopDist; /* lumaFastDistortion, chromaFastDistortion */
SVT_AMD_API int svt_amd_fast_loop_distortion_batch(SvtAmdContext *ctx, const uint8_t *d_src_y, uint32_t srcStrideY,
                                                   const uint8_t *d_src_cb, const uint8_t *d_src_cr, uint32_t srcStrideC,
                                                   const uint8_t *d_pred_y, uint32_t predStrideY, const uint8_t *d_pred_cb,
                                                   const uint8_t *d_pred_cr, uint32_t predStrideC,
                                                   const SvtAmdFastLoopCand *d_cands, uint32_t ncand, SvtAmdFastLoopDist *d_out);

/* ------------------------------------------------------------------------- */
/* Encode-pass inter prediction of prediction units                            */
/* ------------------------------------------------------------------------- */
/* Replaces EncodePassInterPrediction (Codec/EbInterPrediction.c:761-926, called per prediction unit from
 * EbCodingLoop.c:3932) with its EncodeUniPredInterpolation / EncodeBiPredInterpolation (Codec/EbMcp.c:175-250, :562-760)
 * for 8-bit 4:2:0: clamp of the quarter-sample position to the padded picture (:802-812), split into integer and
 * fractional parts for luma (1/4) and chroma (1/8), the HEVC interpolation of the three planes and, for bi-prediction,
 * the average of the two 14-bit intermediates.  Reference pictures are whole padded pictures resident in HBM. */
typedef struct SvtAmdRefPicture {
    const void *d_y, *d_cb, *d_cr;     /* device pointers to the START of the padded buffers (not to sample (0,0))  */
    uint32_t strideY, strideC;         /* in samples                                                               */
    uint32_t originX, originY;         /* luma padding: sample (0,0) is at originX + originY*strideY               */
    uint32_t width, height;            /* luma                                                                     */
} SvtAmdRefPicture;
typedef struct SvtAmdInterPuJob {
    int16_t  mv[2][2];                 /* [list][x, y] in quarter samples                                          */
    uint16_t pu_x, pu_y;               /* luma position of the unit in the picture                                 */
    uint8_t  pu_w, pu_h;               /* 8 .. 64                                                                  */
    uint8_t  pred_dir;                 /* UNI_PRED_LIST_0 0, UNI_PRED_LIST_1 1, BI_PRED 2                          */
    uint8_t  pad;
    int32_t  dst_off_y, dst_off_c;     /* sample offsets of the unit inside the destination planes                 */
} SvtAmdInterPuJob;
/* BATCHED: `jobs` is a HOST array (the call derives the per-plane interpolation lists from it and uploads them);
 * reference pictures and destination planes are device memory.  ref1 may be NULL when no job uses list 1. */
SVT_AMD_API int svt_amd_inter_pu_batch(SvtAmdContext *ctx, const SvtAmdInterPuJob *jobs, uint32_t njobs,
                                       const SvtAmdRefPicture *ref0, const SvtAmdRefPicture *ref1, uint8_t *d_pred_y,
                                       uint32_t strideY, uint8_t *d_pred_cb, uint8_t *d_pred_cr, uint32_t strideC);
/* The 16-bit twin: replaces EncodePassInterPrediction16bit (Codec/EbInterPrediction.c:928-1110) with UniPredInterpolation16bit /
 * BiPredInterpolation16bit (Codec/EbMcp.c:249, :804); reference and destination planes hold 16-bit samples (10-bit content,
 * EbReferenceObject_t.referencePicture16bit), strides and offsets in samples. */
SVT_AMD_API int svt_amd_inter_pu_batch16bit(SvtAmdContext *ctx, const SvtAmdInterPuJob *jobs, uint32_t njobs,
                                            const SvtAmdRefPicture *ref0, const SvtAmdRefPicture *ref1, uint16_t *d_pred_y,
                                            uint32_t strideY, uint16_t *d_pred_cb, uint16_t *d_pred_cr, uint32_t strideC);
/* The mode decision of a 10-bit encode predicts in 8 bits from the 8 MSBs of the 16-bit reference pictures (Inter2Nx2NPuPredictionHevc
 * with is16bit: UnPackReferenceBlock, Codec/EbInterPrediction.c:414-457, 589-760): ref0 / ref1 hold 16-bit planes, the prediction is
 * 8-bit; otherwise as svt_amd_inter_pu_batch. */
SVT_AMD_API int svt_amd_inter_pu_batch_msb(SvtAmdContext *ctx, const SvtAmdInterPuJob *jobs, uint32_t njobs, const SvtAmdRefPicture *ref0,
                                           const SvtAmdRefPicture *ref1, uint8_t *d_pred_y, uint32_t strideY, uint8_t *d_pred_cb,
                                           uint8_t *d_pred_cr, uint32_t strideC);

/* ------------------------------------------------------------------------- */
/* Encode-pass intra prediction of a prediction unit from its neighbours      */
/* ------------------------------------------------------------------------- */
/* Replaces the pair GenerateIntraReferenceSamplesEncodePass (Codec/EbIntraPrediction.c:212-757; 16-bit twin :760-1300)
 * + EncodePassIntraPrediction (:4395-4673; 16-bit :4680-4960) that the encode pass reaches through the global tables
 * GenerateIntraReferenceSamplesFuncTable / EncodePassIntraPredictionFuncTable (Codec/EbCodingLoop.c:1814, :1832):
 * availability of every 4-sample neighbour group (array bound, z-order, slice, picture / tile edge, constrained intra),
 * substitution of the missing ones, [1 2 1] / strong (bilinear) smoothing of the luma reference, filtered-or-not choice by
 * mode and size (intraLumaFilterTable), and the prediction of the luma block and, with the derived chroma mode, of the
 * two chroma blocks (4:2:0).  The job carries the slices of the reference's neighbour arrays the unit can see, already
 * cut out by the caller: entry i of left[] / top[] = i-th sample below / right of the unit's top-left corner. */
typedef struct SvtAmdIntraPuJob {
    uint32_t size;                         /* 8 / 16 / 32; 4 = a luma partition of an intra 4x4 coding unit (luma only; */
                                           /* its chroma pair is the chroma part of a size-8 job at the coding unit)  */
    uint8_t  constrained_intra, strong_smoothing;
    uint8_t  pic_left, pic_top, pic_right; /* pictureLeft/Top/RightBoundary arguments (tile edges)                */
    uint8_t  bottom_left_ok, top_right_ok; /* isBottomLeftAvailable / isUpperRightAvailable(cuDepth, cuIndex)     */
    uint8_t  luma_mode, chroma_mode;       /* EB_INTRA_* / EB_INTRA_CHROMA_* (4 = derived from luma)              */
    uint8_t  mode_tl;                      /* mode-type neighbour entries: 1 INTER, 2 INTRA, 0xFF invalid,        */
    uint8_t  mode_left[16], mode_top[16];  /*   0xFE beyond the array; one per 4 luma samples                     */
    uint8_t  no_smoothing;                 /* 1: never take the filtered reference (IntraPredictionOl, the open-loop  */
    uint8_t  pad;                          /*    mode decision: neighbours = source samples, 128 where there are none) */
    uint16_t left[3][64], top[3][64];      /* [Y, Cb, Cr][i]: reconstructed neighbour samples (chroma: size used)  */
    uint16_t tl[3], pad2;
    int32_t  dst_off_y, dst_off_c;         /* sample offsets of the unit inside the three destination planes      */
} SvtAmdIntraPuJob;
/* BATCHED (device pointers): job j predicts into d_pred_y / d_pred_cb / d_pred_cr at its offsets; strides in samples. */
SVT_AMD_API int svt_amd_intra_pu_batch(SvtAmdContext *ctx, int bytes_per_sample, const SvtAmdIntraPuJob *d_jobs,
                                       uint32_t njobs, void *d_pred_y, uint32_t strideY, void *d_pred_cb, void *d_pred_cr,
                                       uint32_t strideC);
/* Per-call form on HOST pointers (one unit, blocking): the binding of the two table slots, and of the mode decision's
 * IntraPredictionCl (Codec/EbIntraPrediction.c:3682; generators GenerateIntraLuma/ChromaReferenceSamplesMd, EbProductCodingLoop.c:
 * 269, :2196), which asks for the luma block and the chroma pair separately: pred_y == NULL or pred_cb == pred_cr == NULL
 * leaves that part out.  Its open-loop twin IntraPredictionOl (:5427; neighbours = source samples cut by UpdateNeighborSamples
 * ArrayOL / UpdateChromaNeighborSamplesArrayOL, :4952, :5065: mid-grey where the picture ends, no substitution, no smoothing) is
 * the same call with every neighbour group marked available, the literal samples in left / top / tl and no_smoothing = 1. */
SVT_AMD_API int svt_amd_intra_pu(SvtAmdContext *ctx, int bytes_per_sample, const SvtAmdIntraPuJob *job, void *pred_y,
                                 uint32_t strideY, void *pred_cb, void *pred_cr, uint32_t strideC);

/* ------------------------------------------------------------------------- */
/* Device-resident encode pass: hip_encdec_segment                             */
/* ------------------------------------------------------------------------- */
/* The batched boundary of the closed-loop half (SURVEY 8b `hip_encdec_segment`) for the final encode pass: ONE call runs the
 * coding-unit loop of EncodePass (Codec/EbCodingLoop.c:2989, :3180-4594) for every LCU the host declares ready - the LCUs of
 * one wavefront step (AssignEncDecSegments, Codec/EbEncDecProcess.c:1540) - one workgroup per LCU, the units of an LCU in order
 * on the device: intra reference + prediction (GenerateIntraReferenceSamplesEncodePass, EncodePassIntraPrediction), EncodeLoop
 * (residual, Estimate transform, UnifiedQuantizeInvQuantize) and EncodeGenerateRecon of the three planes, neighbour update.
 * The picture's un-deblocked reconstruction and its mode-type map stay on the device between calls (SvtAmdEncDecPicture) and
 * stand in for the reference's ep*NeighborArray set (EbPictureControlSet.h:238-246).
 *
 * EncDec INPUT contract (what the mode decision hands over per LCU: the final coding-unit tree of LargestCodingUnit_t.
 * codedLeafArrayPtr, Codec/EbCodingUnit.h:63-88, 186-222): */
#define SVT_AMD_LCU_MAX_CUS 64
/* what the inter branch of EncodePass does with a unit (EbCodingLoop.c:3817-4400), decided by the host from the mode decision's
 * outputs before the call (mergeFlag, and for merge units skipCost <= mergeCost, :3838-3882): */
#define SVT_AMD_EP_INTER_AMVP  0   /* mergeFlag == 0: EncodeLoop of every transform unit + the luma cbf decision (PictureFullDistortionLuma,
                                    * TuEstimateCoeffBitsEncDec, EncodeTuCalcCost: coded vs. zeroed luma by distortion + lambda * rate)  */
#define SVT_AMD_EP_INTER_MERGE 1   /* merge, not skipped: EncodeLoop of every transform unit, cbf = "has coefficients" (:4164-4253)        */
#define SVT_AMD_EP_INTER_SKIP  2   /* merge decided skip: no residual, the prediction is the reconstruction (:4165-4171)                  */
typedef struct SvtAmdLcuCu {
    uint8_t x, y, size;            /* origin inside the LCU and size in luma samples (GetCodedUnitStats): 8 / 16 / 32; inter units
                                    * also 64 (four 32x32 transform units, tuItr 1..4, EbCodingLoop.c:3944-3970)                 */
    uint8_t pred_mode;             /* CodingUnit_t.predictionModeFlag: 1 INTER_MODE (2Nx2N), 2 INTRA_MODE (2Nx2N)               */
    uint8_t intra_luma_mode;       /* PredictionUnit_t.intraLumaMode, EB_INTRA_PLANAR .. EB_INTRA_MODE_34                  */
    uint8_t bottom_left_ok, top_right_ok; /* isBottomLeftAvailable / isUpperRightAvailable(depth, index), EbAvailability.c */
    uint8_t qp, chroma_qp;         /* cuPtr->qp; MapChromaQp(clip(qp + cbQpOffset + sliceCbQpOffset)) (EbCodingLoop.c:3255) */
    uint8_t leaf_index;            /* index of the unit in codedLeafArrayPtr (0..84)                                       */
    uint8_t inter_dir;             /* PredictionUnit_t.interPredDirectionIndex: UNI_PRED_LIST_0 0, UNI_PRED_LIST_1 1, BI_PRED 2 */
    uint8_t inter_kind;            /* SVT_AMD_EP_INTER_*                                                                   */
    uint32_t dz_offset;            /* dead-zone override of the luma quantiser (EbCodingLoop.c:3092-3133; 0 = none)        */
    int16_t mv[2][2];              /* PredictionUnit_t.mv[list].{x, y}, quarter samples                                    */
} SvtAmdLcuCu;
typedef struct SvtAmdLcuWork {
    uint16_t lcu_x, lcu_y;         /* luma origin of the LCU in the picture                                              */
    uint8_t num_cus;               /* coded leaves (splitFlag == 0) in Z order                                           */
    uint8_t slice_type;            /* EB_PICTURE: 0 B, 1 P, 2 I                                                           */
    uint8_t temporal_layer, constrained_intra, strong_smoothing;
    uint8_t tile_left, tile_top, tile_right; /* lcuEdgeInfoPtr->tileLeft/Top/RightEdgeFlag                              */
    uint8_t pad[4];
    uint32_t full_lambda;          /* contextPtr->fullLambda of the LCU (EncDecConfigureLcu, EbEncDecProcess.c:1448): inter units  */
    uint32_t luma_cbf_bits[4];     /* mdRateEstimationPtr->lumaCbfBits[ctx], [ctx + (NUMBER_OF_CBF_CASES >> 1)] for ctx 0, 1:
                                    * {zero cbf ctx 0, zero cbf ctx 1, non-zero ctx 0, non-zero ctx 1} (EncodeTuCalcCost)         */
    uint8_t pm_core;               /* contextPtr->mdContext->rdoqPmCoreMethod == EB_PMCORE (encMode 1..4): the quantiser of every unit is
                                    * DecoupledQuantizeInvQuantizeLoops (Codec/EbTransforms.c:3009-3052): no dead-zone override, luma levels
                                    * re-decided per 4x4 block by SSE + full_lambda * rate (needs the picture's rate tables)           */
    uint8_t pad2[11];
    SvtAmdLcuCu cu[SVT_AMD_LCU_MAX_CUS];
    uint8_t src_y[64 * 64], src_cb[32 * 32], src_cr[32 * 32]; /* source samples of the LCU (enhancedPicturePtr), pitch 64 / 32 */
} SvtAmdLcuWork;
/* EncDec OUTPUT contract (what entropy coding and the loop filters need back per LCU): the TransformUnit_t fields the encode
 * loop sets (Codec/EbTransformUnit.h:18-37), LargestCodingUnit_t.quantizedCoeff (s16, 64-pitch Y + two 32-pitch chroma planes at
 * LCU-local positions) and the un-deblocked reconstruction of the LCU. */
typedef struct SvtAmdLcuCuResult {
    uint8_t cbf[3];                /* lumaCbf, cbCbf, crCbf                       */
    uint8_t only_dc[3];            /* isOnlyDc[0..2]                              */
    uint16_t nz[3];                /* nzCoefCount[0..2]                           */
} SvtAmdLcuCuResult;
typedef struct SvtAmdLcuResult {
    SvtAmdLcuCuResult cu[SVT_AMD_LCU_MAX_CUS];           /* by position in SvtAmdLcuWork.cu */
    int16_t coeff_y[64 * 64], coeff_cb[32 * 32], coeff_cr[32 * 32];
    uint8_t rec_y[64 * 64], rec_cb[32 * 32], rec_cr[32 * 32]; /* inside the picture only */
} SvtAmdLcuResult;
/* 16-bit twins (EncodePass with is16bit: 10-bit samples in uint16_t; the source of an LCU is contextPtr->inputSample16bitBuffer as
 * EncodePassPackLcu, EbCodingLoop.c:2867, leaves it; the quantiser runs at qp + QP_BD_OFFSET, :1307) */
typedef struct SvtAmdLcuWork16 {
    uint16_t lcu_x, lcu_y;
    uint8_t num_cus, slice_type, temporal_layer, constrained_intra, strong_smoothing;
    uint8_t tile_left, tile_top, tile_right;
    uint8_t pad[4];
    uint32_t full_lambda;
    uint32_t luma_cbf_bits[4];
    uint8_t pm_core;
    uint8_t pad2[11];
    SvtAmdLcuCu cu[SVT_AMD_LCU_MAX_CUS];
    uint16_t src_y[64 * 64], src_cb[32 * 32], src_cr[32 * 32];
} SvtAmdLcuWork16;
typedef struct SvtAmdLcuResult16 {
    SvtAmdLcuCuResult cu[SVT_AMD_LCU_MAX_CUS];
    int16_t coeff_y[64 * 64], coeff_cb[32 * 32], coeff_cr[32 * 32];
    uint16_t rec_y[64 * 64], rec_cb[32 * 32], rec_cr[32 * 32];
} SvtAmdLcuResult16;
typedef struct SvtAmdEncDecPicture SvtAmdEncDecPicture;
SVT_AMD_API int svt_amd_encdec_picture_create(SvtAmdContext *ctx, uint16_t luma_width, uint16_t luma_height, int bytes_per_sample,
                                              SvtAmdEncDecPicture **out);
SVT_AMD_API int svt_amd_encdec_picture_begin(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic); /* new picture: nothing coded yet */
/* P / B pictures: the picture-level inputs of the inter units (EncodePassInterPrediction reads pictureControlSetPtr->refPicPtrArray[list],
 * Codec/EbInterPrediction.c:761; TuEstimateCoeffBitsEncDec reads pictureControlSetPtr->cabacCost, EbCodingLoop.c:4103) - reference
 * pictures of list 0 / 1 (DEVICE planes, whole padded buffers of the picture's size and sample width; either or - for an I picture that only
 * needs the rate tables, SvtAmdLcuWork.pm_core - both may be NULL) and the
 * coefficient-rate tables (HOST pointer, copied on the context's stream).  Call before the first LCU with inter units; holds until the
 * next call for this picture object. */
SVT_AMD_API int svt_amd_encdec_picture_set_inter(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdRefPicture *ref0,
                                                 const SvtAmdRefPicture *ref1, const SvtAmdCabacCost *cost);
SVT_AMD_API int svt_amd_encdec_picture_destroy(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic);
/* works / results: HOST arrays of n LCUs that do not depend on each other (left, top and top-right LCUs of each were encoded by
 * earlier calls); blocking.  Lanes of one context family may call concurrently for different LCUs of one picture. */
SVT_AMD_API int svt_amd_encode_lcus(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *works, int n,
                                    SvtAmdLcuResult *results);

/* the same for a picture created with bytes_per_sample = 2 */
SVT_AMD_API int svt_amd_encode_lcus16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *works, int n,
                                      SvtAmdLcuResult16 *results);

/* The whole picture in ONE call: works / results are HOST arrays of every LCU of the picture in raster order.  The wavefront of
 * AssignEncDecSegments (Codec/EbEncDecProcess.c:1540; an LCU starts when its left and top-right LCUs of the same tile are done) runs
 * on the device - workgroups draw LCUs in raster order and wait for their neighbours' completion flags - so the host makes no
 * scheduling decision and the picture costs one launch.  Implies svt_amd_encdec_picture_begin.  Blocking. */
SVT_AMD_API int svt_amd_encode_picture(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *works, SvtAmdLcuResult *results);
SVT_AMD_API int svt_amd_encode_picture16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *works, SvtAmdLcuResult16 *results);
/* The same on DEVICE arrays (the unit lists are not validated); asynchronous on the context's stream.  tiles: tiles of the picture
 * (they run side by side; sizes the persistent grid). */
SVT_AMD_API int svt_amd_encode_picture_device(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *d_works,
                                              SvtAmdLcuResult *d_results, int tiles);
/* An LCU waits only for what its units read across its border: intra units read the left / top-left / top / top-right LCU's reconstruction
 * and mode types, inter units nothing (they predict from the reference pictures).  LCUs without an intra unit - most LCUs of a P / B picture -
 * therefore start at once, on as many workgroups as the device holds.  The host-array calls above count such LCUs themselves; this device-array
 * form is told: free_lcus = number of LCUs without an intra unit. */
SVT_AMD_API int svt_amd_encode_picture_device_inter(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *d_works,
                                                    SvtAmdLcuResult *d_results, int tiles, int free_lcus);

/* Multi-GPU over tiles (tiles are independent inside a picture: EncDec never reads across a tile edge, Codec/EbEncDecProcess.c:2743-2760,
 * and the in-loop filters do not cross one either - loop_filter_across_tiles_enabled_flag is written 0, Codec/EbEntropyCoding.c:6346-6351).  A rank's
 * picture:   svt_amd_encode_picture_rect[16]  - works / results as in svt_amd_encode_picture (every LCU's unit list; tile-edge flags), only the LCUs
 *              inside `rect` (the rank's rectangle of whole tiles, svt_amd_tile_partition) are encoded, on the same device wavefront; the other
 *              LCUs' results come back zeroed;
 *            svt_amd_encdec_picture_deblock / _sao as on one GPU (the rank's rectangle comes out finished, the rest is not meaningful);
 *            svt_amd_encdec_picture_exchange   - the object's latest stage completed across ranks: own rectangle out, the others' in (one
 *              ncclAllGather, svt_amd_recon_exchange); _pack is its local half for hosts with their own transport (svt_amd_recon_pack);
 *            svt_amd_encdec_picture_reference  - the now complete picture padded: the next pictures' reference on every rank. */
SVT_AMD_API int svt_amd_encode_picture_rect(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *works, SvtAmdLcuResult *results,
                                            const SvtAmdRect *rect);
SVT_AMD_API int svt_amd_encode_picture_rect16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *works, SvtAmdLcuResult16 *results,
                                              const SvtAmdRect *rect);
/* the same restriction for the object's MODE-DECISION calls (svt_amd_md_encode_picture / _inter: mode decision + encode pass of the rank's rectangle in one call;
 * the rectangle's borders must be tile borders of the SvtAmdMdLcu records; the other LCUs' records come back zeroed); rect NULL = the whole picture */
SVT_AMD_API int svt_amd_encdec_picture_set_rect(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdRect *rect);
SVT_AMD_API int svt_amd_encdec_picture_exchange(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdRect *rects, int world, int rank);
/* Multi-GPU over PICTURES (SURVEY 8e last row): the pictures of a mini-GOP are owned by different ranks - the two non-reference B pictures of temporal layer 2 run at
 * the same time on two ranks - and a rank encodes the whole of its picture (svt_amd_encode_picture* / svt_amd_md_encode_picture*, deblocking, SAO); the only traffic is
 * the finished REFERENCE picture, sent by its owner once:
 *   svt_amd_encdec_picture_broadcast - ncclBroadcast of the object's latest stage from rank `root` (communicator of svt_amd_comm_init); on the other ranks the planes
 *     land in the object's final stage, svt_amd_encdec_picture_reference then pads the picture there as on its owner;
 *   svt_amd_encdec_picture_import    - the same hand-over between two picture objects of one process (logical ranks on one device, a host with its own transport):
 *     a copy on ctx's stream, ordered BEHIND whatever last wrote `from` (the event recorded behind its encode pass, filter or exchange).  It does not hold `from`'s owner
 *     back: the owner must not start its next picture on `from` before the importer's stream has passed the copy (svt_amd_lane_event_record / _wait, or
 *     svt_amd_synchronize on the importer's context);
 *   svt_amd_recon_broadcast          - the collective on caller-owned planes (whole allocations of bytes[p] bytes, equal on every rank). */
SVT_AMD_API int svt_amd_recon_broadcast(SvtAmdContext *ctx, void *const d_planes[3], const size_t bytes[3], int world, int rank, int root);
SVT_AMD_API int svt_amd_encdec_picture_broadcast(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int world, int rank, int root);
SVT_AMD_API int svt_amd_encdec_picture_import(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdEncDecPicture *from);
SVT_AMD_API int svt_amd_encdec_picture_pack(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdRect *rects, int world, int r, void *d_slots,
                                            size_t slot_bytes, int to_slot);

/*
 * Entropy hand-off pre-scan.  What EncodeQuantizedCoefficients (Codec/EbEntropyCoding.c:1172; callers EncodeCoeff :4069,
 * EncodeTuCoeff :4210) does with a transform block BEFORE it codes a single bin is data parallel and needs nothing but the block: the mode-dependent
 * scan (:1347-1372), the coefficients re-ordered by sub-block and scan with a significance map per 4x4 sub-block (:1378-1430), the last
 * significant position (:1432-1461) - and the sign / greater-than-1 patterns its level loop derives from the same values (:1532-1600).  The device
 * holds every quantizedCoeff after the encode pass, so it hands the entropy coder these instead of 3 * W * H / 2 bytes of s16 planes:
 *   per transform block  SvtAmdCoeffScanTu (8 B): scan, last sub-block, last position, DC-only fast track (:1308), where its sub-blocks start;
 *   per 4x4 sub-block    SvtAmdCoeffScanGroup (8 B), sub-blocks lastScanSet .. 0 in CODING order (empty ones too: their coded_sub_block_flag is
 *                        coded): significance map in forward scan order, sign bits and |level| > 1 flags of the coded coefficients (CODING
 *                        order = set bits of the map from the highest position down; `sign` holds popcount(sigmap) bits right-aligned, the first
 *                        coded coefficient at bit popcount - 1; the first coded coefficient sits in bit 0 of `gt1`), index of its first level;
 *   per coefficient      its absolute level (u16), non-zero coefficients only, CODING order.
 * The CABAC loop that consumes them codes exactly the reference's bins: integration/svt_coeff_scan_consumer.h.
 * Blocks: slot c of component p = the unit at position c of SvtAmdLcuWork.cu (luma: the unit's size; chroma: half of it, 4x4 for an 8x8
 * unit); a 64x64 unit's four transform units are slots 1..4 (as in SvtAmdLcuResult.cu).  last_scan_set = -1: nothing to code (cbf 0).
 */
typedef struct SvtAmdCoeffScanTu {
    uint8_t scan_index;            /* SCAN_DIAG2 0 / SCAN_HOR2 1 / SCAN_VER2 2 (Codec/EbEntropyCodingUtil.h:43)                   */
    int8_t last_scan_set;          /* lastScanSet; -1 = no non-zero coefficient                                                   */
    uint8_t pos_last;              /* posLast: scan position of the last significant coefficient inside that sub-block            */
    uint8_t last_x, last_y;        /* lastSigXPos / lastSigYPos as EncodeLastSignificantXY takes them (swapped for SCAN_HOR2 / _VER2) */
    uint8_t dc_only;               /* numNonZeroCoeffs == 1 && coeff[0] != 0: the fast track of :1308-1344 (one group, one level)  */
    uint16_t first_group;          /* index of the block's first group in the LCU's group list                                    */
} SvtAmdCoeffScanTu;
typedef struct SvtAmdCoeffScanGroup {
    uint16_t sigmap;               /* bit k: the k-th coefficient of the sub-block in forward scan order is non-zero               */
    uint16_t sign;                 /* signFlags of :1547-1600: n = popcount(sigmap) sign bits, RIGHT-aligned: the first coded coefficient  */
                                   /* at bit n - 1, the last at bit 0 (what EncodeBypassBins(sign, n) writes first / last)                 */
    uint16_t gt1;                  /* bit i: the i-th coded coefficient has |level| > 1                                           */
    uint16_t first_level;          /* index of the sub-block's first level in the LCU's level list                                */
} SvtAmdCoeffScanGroup;
typedef struct SvtAmdCoeffScanLcu {
    uint32_t group_base, level_base; /* where the LCU's groups / levels start in the picture's lists                              */
    uint16_t groups, levels;         /* how many it has (<= 384 / <= 6144)                                                         */
    uint8_t pad[4];
    SvtAmdCoeffScanTu tu[3][SVT_AMD_LCU_MAX_CUS];       /* [Y, Cb, Cr][slot]                                                       */
} SvtAmdCoeffScanLcu;
/* One call per picture.  works / results: the encode pass's records of n_lcus LCUs - HOST arrays (device_arrays 0; uploaded) or DEVICE arrays
 * (device_arrays 1: what svt_amd_encode_picture_device / svt_amd_md_encode_picture left in HBM); work_stride / result_stride: sizeof the record
 * type (the 8- and 16-bit records share their heads, coefficients are s16 in both).  Outputs (HOST): lcus[n_lcus]; groups / levels: the
 * picture's lists, compacted in LCU order - capacities in elements (worst case 384 / 6144 per LCU); totals[2] = {groups, levels} written.
 * SVT_AMD_ERR_RESOURCES when a capacity is too small (totals then tell what is needed).  Blocking.
 * HOST arrays may lie at any address and stride; only the first 1584 bytes of a work record and the offsetof(rec_y) bytes in front of a result record's
 * reconstruction are uploaded.  DEVICE arrays are read in place, by words: both arrays 4-byte aligned, both strides multiples of 4 (and, as for host arrays, at
 * least 1584 / offsetof(rec_y)) - every sizeof of the record types and every hipMalloc pointer keeps that rule; anything else is SVT_AMD_ERR_BAD_PARAM.
 * The call runs the kernels of the stream-ordered launch below into the context's scratch (head, lcus, the lists up to min(capacity, worst case), the uploaded
 * heads) and keeps what is its own: these checks, the upload, the downloads, the waits, the return codes.  n_lcus has no upper limit here.
 * Malformed records (a bad LCU or a bad unit as the launch below counts them) are refused: SVT_AMD_ERR_BAD_PARAM, judged before the capacities;
 * svt_amd_last_error names this entry, both counts, the first bad LCU and the first LCU with a bad unit (-1: none).  As with SVT_AMD_ERR_RESOURCES, totals and
 * lcus[] are written (a refused LCU or unit reads "nothing to code") and groups / levels are not touched. */
SVT_AMD_API int svt_amd_coeff_scan_picture(SvtAmdContext *ctx, const void *works, size_t work_stride, const void *results, size_t result_stride,
                                           int device_arrays, int n_lcus, SvtAmdCoeffScanLcu *lcus, SvtAmdCoeffScanGroup *groups,
                                           uint32_t group_capacity, uint16_t *levels, uint32_t level_capacity, uint32_t totals[2]);
/* The same hand-off as a STREAM-ORDERED LAUNCH on the records in HBM, the last stage of the per-picture chain (svt_amd_md_encode_picture_launch,
 * svt_amd_encdec_picture_tail_launch, then this): everything is queued on ctx's stream and the call returns.  It synchronises nothing, copies nothing from or to
 * host memory and waits for no event.  It has no working memory: it never touches the context's scratch, and everything it needs between its three kernels lies in
 * the caller's output arrays (the per-LCU counts are fields of SvtAmdCoeffScanLcu), so launches into different output arrays may be in flight together.  The only
 * thing the first call on a device does that later calls do not is the upload of the immutable scan tables.  svt_amd_coeff_scan_picture above runs these kernels too.
 *   Outputs (every pointer DEVICE memory; nothing behind n_lcus records or behind either capacity is ever written).  On well-formed records lcus[] with its
 *   bases, groups[0 .. head.groups), levels[0 .. head.levels) and {head.groups, head.levels} are byte for byte what svt_amd_coeff_scan_picture returns: the same
 *   lists packed in LCU order.  work_heads / result_heads (optional) receive the first 1584 / 768 bytes of every record - head and unit list, cbf and count
 *   records: what the entropy coder reads besides the lists - of refused LCUs too: a copy, not a judgement.
 *   Overflow is no failure the host could see - the call has returned by then: head carries the totals the picture NEEDS and the overflow bits; an LCU whose
 *   group range [group_base, group_base + groups) fits the capacity has its groups written, one whose level range fits has its levels written, each list judged on
 *   its own; lcus[] is complete in either case, so the caller can launch again with the capacities head names.
 *   The records are not validated on the host; what a host loop would refuse is COUNTED in head, as SvtAmdTailCheck counts (first_* 0xFFFFFFFF: none).
 *     A bad LCU: num_cus > 64, or its well-formed units cover more than 64x64 samples together (they overlap: the lists of an LCU hold 384 sub-blocks).  It has no
 *     block: groups = levels = 0 and every tu says "nothing to code" (last_scan_set -1, everything else 0).  Its units are not counted.
 *     A bad unit: its size is not 8 / 16 / 32 / 64, or x or y is not a multiple of 8, or it leaves the LCU, or it is a 64x64 unit that is not the only unit of its
 *     LCU at (0, 0).  None of its three blocks is scanned; its slots read "nothing to code".
 *     No access leaves the record arrays, whatever the records hold.
 *   Everything the host can judge is checked before anything is queued: NULL required pointers, alignment, strides, n_lcus, non-zero pads, a picture object of
 *   another device.  A refusal names the entry in svt_amd_last_error and queues nothing. */
typedef struct SvtAmdEntropyHandoffHead {      /* 32 bytes, written once per launch */
    uint32_t groups, levels;                   /* what the picture NEEDS (whether or not it fitted) */
    uint32_t overflow;                         /* bit 0: groups > group_capacity, bit 1: levels > level_capacity */
    uint32_t bad_lcus, first_bad_lcu;          /* as SvtAmdTailCheck: 0xFFFFFFFF = none */
    uint32_t bad_units, first_bad_unit_lcu;
    uint32_t pad;                              /* written as 0 */
} SvtAmdEntropyHandoffHead;
typedef struct SvtAmdEntropyHandoffJob {
    const void *d_works;  size_t work_stride;  /* DEVICE SvtAmdLcuWork[16], 4-byte aligned; stride a multiple of 4, >= the head + unit list (1584) */
    const void *d_results; size_t result_stride;/* DEVICE SvtAmdLcuResult[16], 4-byte aligned; stride a multiple of 4, >= offsetof(rec_y) */
    uint32_t n_lcus;                           /* 1 .. SVT_AMD_MDCTL_MAX_LCUS */
    uint32_t group_capacity, level_capacity;   /* elements of out.groups / out.levels */
    uint32_t pad;                              /* 0 */
} SvtAmdEntropyHandoffJob;
typedef struct SvtAmdEntropyHandoffOut {       /* every pointer DEVICE memory */
    SvtAmdEntropyHandoffHead *head;            /* required, 4-byte aligned */
    SvtAmdCoeffScanLcu *lcus;                  /* required, [n_lcus], 4-byte aligned */
    SvtAmdCoeffScanGroup *groups;              /* required, [group_capacity], 8-byte aligned */
    uint16_t *levels;                          /* required, [level_capacity] */
    void *work_heads;                          /* optional: [n_lcus][1584], the head and unit list of every work record, tight; 4-byte aligned */
    SvtAmdLcuCuResult *result_heads;           /* optional: [n_lcus][SVT_AMD_LCU_MAX_CUS], tight; 4-byte aligned */
} SvtAmdEntropyHandoffOut;
#define SVT_AMD_ENTROPY_HANDOFF_HEAD 0
#define SVT_AMD_ENTROPY_HANDOFF_LCUS 1
#define SVT_AMD_ENTROPY_HANDOFF_GROUPS 2
#define SVT_AMD_ENTROPY_HANDOFF_LEVELS 3
#define SVT_AMD_ENTROPY_HANDOFF_WORK_HEADS 4
#define SVT_AMD_ENTROPY_HANDOFF_RESULT_HEADS 5
/* bytes of the output arrays of a picture: _HEAD 32, _LCUS LCUs * sizeof(SvtAmdCoeffScanLcu), _GROUPS the worst case of 384 groups an LCU, _LEVELS the worst
 * case of 6144 levels an LCU, _WORK_HEADS LCUs * 1584, _RESULT_HEADS LCUs * 768; 0 for anything else.  Host arithmetic: no context, no device. */
SVT_AMD_API size_t svt_amd_entropy_handoff_bytes(uint16_t luma_width, uint16_t luma_height, int which);
SVT_AMD_API int svt_amd_entropy_handoff_launch(SvtAmdContext *ctx, const SvtAmdEntropyHandoffJob *job, const SvtAmdEntropyHandoffOut *out);
/* The object form: the records the LAST svt_amd_md_encode_picture[_inter][16] call or launch left on `pic`, and the object's number of LCUs.  Refused exactly where
 * svt_amd_encdec_picture_motion_field is refused - no completed call, a P / B call that decided only, an object with a rank rectangle
 * (svt_amd_encdec_picture_set_rect) - and on a picture object of another device.  Queued on ctx's stream: on the context that call ran on, stream order suffices. */
SVT_AMD_API int svt_amd_encdec_picture_entropy_handoff(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, uint32_t group_capacity, uint32_t level_capacity,
                                                       const SvtAmdEntropyHandoffOut *out);

/* Deblocking behind the encode pass: when every LCU of the picture is encoded, a copy of the device picture (a second set of planes of
 * the picture object; the un-deblocked planes stay as they are) goes through the
 * picture-level boundary-strength and deblocking kernels (svt_amd_bs_picture + svt_amd_dlf_picture: the state the reference's
 * per-LCU drivers LCUInternalAreaDLFCore / LCUBoundaryDLFCore / LCUPictureEdgeDLFCore leave, Codec/EbCodingLoop.c:4600-4631) -
 * the finished reconstruction / reference picture when SAO is off.  works / results: the HOST records of all LCUs in raster
 * order (unit lists, QPs, tile edges; luma cbf of every unit).  out_*: optional HOST planes (tight pitch) that receive the
 * deblocked picture.  Blocking. */
typedef struct SvtAmdDeblockParams {
    int8_t tc_offset, beta_offset, cb_qp_offset, cr_qp_offset;   /* pictureControlSetPtr->tcOffset / betaOffset / cbQpOffset / crQpOffset */
    uint8_t slice_type;                                           /* EB_PICTURE: 0 B, 1 P, 2 I, 3 IDR */
    uint8_t pad[3];
    uint64_t ref_poc[2];                                          /* refPOC of the two lists (inter units; 0 for intra pictures) */
} SvtAmdDeblockParams;
SVT_AMD_API int svt_amd_encdec_picture_deblock(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *works,
                                               const SvtAmdLcuResult *results, const SvtAmdDeblockParams *params, uint8_t *out_y,
                                               uint8_t *out_cb, uint8_t *out_cr);
SVT_AMD_API int svt_amd_encdec_picture_deblock16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *works,
                                                 const SvtAmdLcuResult16 *results, const SvtAmdDeblockParams *params, uint16_t *out_y,
                                                 uint16_t *out_cb, uint16_t *out_cr);
/* SAO behind the deblocked device picture (after svt_amd_encdec_picture_deblock[16]): statistics of every LCU as the reference's
 * SaoGenerationDecision(16bit) gathers them inside EncodePass (Codec/EbCodingLoop.c:4640-4750, on the picture as it stands when the LCU is
 * done: deblocked, except the last 4 columns / rows of the LCU where a neighbour follows - taken from the un-deblocked picture the object
 * keeps), the parameter decision of the whole picture (svt_amd_sao_decide_picture) and ApplySaoOffsetsPicture (svt_amd_sao_apply_picture)
 * on the deblocked picture.  What is left in the picture object - and copied to out_* (HOST, tightly packed, NULL = not wanted) - is the
 * encoder's finished reconstruction: a reference picture is completed without leaving HBM.  params: the picture's rate inputs; enable:
 * HOST, one byte per LCU (NULL = all 1), 0 where the encode pass shuts SAO off (:4678-4707); lcu_params (HOST, optional): the decided
 * parameters of every LCU (what entropy coding needs).  Blocking. */
SVT_AMD_API int svt_amd_encdec_picture_sao(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork *works,
                                           const SvtAmdSaoDecisionParams *params, const uint8_t *enable, SvtAmdSaoLcuParams *lcu_params,
                                           uint8_t *out_y, uint8_t *out_cb, uint8_t *out_cr);
SVT_AMD_API int svt_amd_encdec_picture_sao16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *works,
                                             const SvtAmdSaoDecisionParams *params, const uint8_t *enable, SvtAmdSaoLcuParams *lcu_params,
                                             uint16_t *out_y, uint16_t *out_cb, uint16_t *out_cr);
/* The parameter decision alone, on the picture object as it stands: after svt_amd_encdec_picture_deblock the encoder-order view as above;
 * without it the picture as encoded - contextPtr->allowEncDecMismatch pictures (Codec/EbEncDecProcess.c:2036-2054: temporal layers > 0 at
 * encMode >= 8, and at encMode 7 in 4K), which the reference neither deblocks nor SAO-filters on its side while it still decides (on the
 * un-deblocked reconstruction) and signals the parameters.  works: SvtAmdLcuWork[] or SvtAmdLcuWork16[] by the picture's sample width. */
SVT_AMD_API int svt_amd_encdec_picture_sao_decide(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const void *works,
                                                  const SvtAmdSaoDecisionParams *params, const uint8_t *enable, SvtAmdSaoLcuParams *lcu_params);
/* The picture object's latest stage (after SAO, else deblocked, else as encoded) as a padded reference picture in HBM - PadRefAndSetFlags
 * (Codec/EbEncDecProcess.c:1805: GeneratePadding[16Bit], edge replication) - in the form svt_amd_encdec_picture_set_inter of a LATER picture
 * object takes: reference pictures never leave the device.  origin_x / origin_y: luma padding (the reference: LCU size + 16 = 80; even);
 * planes are (width + 2 origin_x) samples wide, chroma half of everything.  out_*: optional HOST copies of the padded planes.  *ref stays
 * valid until the picture object is destroyed or the call is repeated on it. */
SVT_AMD_API int svt_amd_encdec_picture_reference(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, uint32_t origin_x, uint32_t origin_y,
                                                 SvtAmdRefPicture *ref, void *out_y, void *out_cb, void *out_cr);

/* ------------------------------------------------------------------------- */
/* Picture tail on the device: deblocking, SAO and padding from the records in HBM */
/* ------------------------------------------------------------------------- */
/* The three blocking entries above take HOST records: they walk every unit of every LCU on the host, upload the maps and (for SAO) the whole work array again, and
 * synchronise five times a reference picture.  The records are in HBM already - the device-array encode entries and the mode-decision calls leave them there - so the
 * tail below derives the filters' inputs from them ON the device and queues the same chain without touching the host.  What the reference does is what the blocking
 * entries cite: LCUInternalAreaDLFCore / LCUBoundaryDLFCore / LCUPictureEdgeDLFCore (Codec/EbDeblockingFilter.c:2222, 2828, 3518; Codec/EbCodingLoop.c:4600-4631) on
 * the strengths of SetBSArrayBasedOnPUBoundary / TUBoundary (:339, :472); SaoGenerationDecision[16bit] (Codec/EbCodingLoop.c:4640-4750,
 * Codec/EbSampleAdaptiveOffsetGenerationDecision.c:647-850, :936-1140); ApplySaoOffsetsPicture (Codec/EbEncDecProcess.c:522-757); PadRefAndSetFlags
 * (Codec/EbEncDecProcess.c:1805).  The blocking entries keep their code and behaviour; on the same inputs the tail leaves the same bytes: the deblocked planes, the
 * finished planes, the parameters, the padded reference.
 *
 * Inputs derived per LCU (tests/tail_numpy.py restates them; svt-hevc_amd/csrc/tail_logic.h is the one text the device and a plain C program compile):
 *   SvtAmdCuMapEntry per 8x8 block (mode and size_log2 of the covering unit; dir and mv of inter units only; everything else 0), QP per 8x8 block, luma cbf per 4x4
 *   block (a 64x64 unit: result slots c + 1 .. c + 4, one per 32x32 quadrant), picture-sized as the filter kernels read them; where two units cover a cell the later one
 *   in list order wins; a cell no unit covers is 0;
 *   per LCU the deblocking edge byte (tile_left | tile_top << 1), SvtAmdSaoLcuParams.edge_flags (1 left, 2 right, 4 top, 8 bottom: the last LCU row, or the LCU
 *   below has tile_top) and the follow bits of the encoder-order composite (1: an LCU of the same tile follows to the right, 2: below);
 *   the LCUs' source samples as three planes.
 * The records are not validated on the host; what the host loops refuse is COUNTED: an LCU that is not at its raster position or has num_cus > 64 (none of its units
 * is taken, its source samples are not scattered), and a unit whose size is not 8 / 16 / 32 / 64, that leaves its LCU or the picture, or - a 64x64 unit - whose result
 * slots leave the record.  An offending unit writes nothing (its cells stay 0); no access leaves the arrays.  first_* are 0xFFFFFFFF when there is none. */
typedef struct SvtAmdTailCheck { uint32_t bad_lcus, first_bad_lcu, bad_units, first_bad_unit_lcu; } SvtAmdTailCheck;
#define SVT_AMD_TAIL_DEBLOCK    1u  /* boundary strengths + deblocking: the object's deblocked planes                                                     */
#define SVT_AMD_TAIL_SAO_DECIDE 2u  /* statistics + parameter decision; without SVT_AMD_TAIL_DEBLOCK on the picture as encoded (allowEncDecMismatch pictures) */
#define SVT_AMD_TAIL_SAO_APPLY  4u  /* the finished planes; needs SVT_AMD_TAIL_SAO_DECIDE and SVT_AMD_TAIL_DEBLOCK in the same job                         */
#define SVT_AMD_TAIL_REFERENCE  8u  /* the latest stage padded (origin_x / origin_y: luma padding, even, 8..256); needs `ref`                                */
typedef struct SvtAmdTailJob {
    const void *d_works;                   /* DEVICE: SvtAmdLcuWork[16] of every LCU, raster order; 4-byte aligned (16-byte aligned records are scattered 16 bytes a lane) */
    size_t      work_stride;               /* any multiple of 4 that holds the record type of the object's sample width                                        */
    const void *d_results;                 /* DEVICE: SvtAmdLcuResult[16]; only cu[].cbf[0] is read                                                           */
    size_t      result_stride;
    const uint8_t *d_sao_enable;           /* DEVICE, one byte an LCU as svt_amd_sao_decide_picture takes it, or NULL = all 1                                 */
    SvtAmdDeblockParams deblock;
    SvtAmdSaoDecisionParams sao;
    uint32_t    origin_x, origin_y;        /* SVT_AMD_TAIL_REFERENCE                                                                                          */
    uint32_t    stages;                    /* SVT_AMD_TAIL_*                                                                                                  */
    uint32_t    pad;                       /* 0                                                                                                               */
} SvtAmdTailJob;
#define SVT_AMD_TAIL_LCU_PARAMS 0
#define SVT_AMD_TAIL_CHECK 1
/* bytes of the optional outputs: SVT_AMD_TAIL_LCU_PARAMS LCUs * sizeof(SvtAmdSaoLcuParams), SVT_AMD_TAIL_CHECK sizeof(SvtAmdTailCheck); 0 for anything else */
SVT_AMD_API size_t svt_amd_picture_tail_bytes(uint16_t luma_width, uint16_t luma_height, int which);
/* Queues the stages of job->stages on ctx's stream behind whatever encoded the picture there, and returns: no synchronisation, no copy from or to the host (the two
 * parameter structs travel by value), no allocation after the first call on the object (or after the warm-up below).  The working memory - maps, both strength
 * arrays, source and composite planes, statistics, parameters, costs - belongs to the picture object and is freed with it: tails of two objects on two lanes can be
 * in flight together.  d_works == NULL && d_results == NULL: the records the LAST svt_amd_md_encode_picture[_inter][16] call left on the object, refused as
 * svt_amd_encdec_picture_motion_field refuses (no completed call, a P / B call without works and results, an object with a rank rectangle).
 * d_lcu_params (DEVICE, optional): the decided SvtAmdSaoLcuParams of every LCU; d_check (DEVICE, optional): one SvtAmdTailCheck (written when a filter stage runs);
 * nothing behind either is written.  ref (HOST, required with SVT_AMD_TAIL_REFERENCE) is filled at queue time, as svt_amd_encdec_picture_reference fills it; the planes
 * are ready in stream order.  The object's deblocked / finished state is set as the blocking calls set it.  Everything is checked before anything is queued: a refusal
 * names the entry in svt_amd_last_error and writes nothing. */
SVT_AMD_API int svt_amd_encdec_picture_tail_launch(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdTailJob *job, SvtAmdSaoLcuParams *d_lcu_params,
                                                   SvtAmdTailCheck *d_check, SvtAmdRefPicture *ref);
/* everything the first tail on the object would allocate, made now; origin_x = origin_y = 0: without the padded reference planes */
SVT_AMD_API int svt_amd_encdec_picture_tail_warmup(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, uint32_t origin_x, uint32_t origin_y);
/* the 16-bit twins of svt_amd_encode_picture_device / svt_amd_encode_picture_device_inter: a 10-bit sequence stays on the device as an 8-bit one does */
SVT_AMD_API int svt_amd_encode_picture_device16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *d_works, SvtAmdLcuResult16 *d_results,
                                                int tiles);
SVT_AMD_API int svt_amd_encode_picture_device_inter16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuWork16 *d_works,
                                                      SvtAmdLcuResult16 *d_results, int tiles, int free_lcus);
/* debug / test: what the object's last tail with a filter stage derived from the records, downloaded (blocking); every pointer HOST and optional.  map / cbf / qp:
 * picture-sized as above; lcu_bytes: [4][LCUs] - deblocking edge byte, SAO edge flags, follow bits, status byte (0x80: the LCU is refused, else its number of
 * refused units); check: the reduced record; src_*: the source planes, tightly packed, of the object's sample width */
SVT_AMD_API int svt_amd_debug_picture_tail_maps(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, SvtAmdCuMapEntry *map, uint8_t *cbf, uint8_t *qp, uint8_t *lcu_bytes,
                                                SvtAmdTailCheck *check, void *src_y, void *src_cb, void *src_cr);

/* debug: out == NULL arms per-LCU shader-clock sums in the encode-pass kernels (16 x u64 per LCU: prediction, encode, copy-out, units,
 * wait for neighbours, start, end, -, the prediction's four sub-phases, 4 unused), a later call with a HOST buffer of 16 * LCUs u64
 * fetches them (tools/encodepass_bench.py) */
SVT_AMD_API int svt_amd_debug_encdec_profile(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out);

/* LCUs the HOST encoded itself (units outside this revision: inter, intra 4x4, 64x64, delta-QP / masking configurations) are
 * handed to the device picture afterwards so that later LCUs find their neighbours: the un-deblocked last row and last column of
 * the LCU and the mode type of the 4x4 cells along them - what the reference's ep*ReconNeighborArray / epModeTypeNeighborArray
 * top and left entries hold when EncodePass returns (EncodePassUpdateReconSampleNeighborArrays, EbCodingLoop.c:1913). */
typedef struct SvtAmdLcuBorder {
    uint16_t lcu_x, lcu_y;
    uint8_t mode_bottom[16], mode_right[16];   /* 1 INTER_MODE / 2 INTRA_MODE per 4 luma samples, left to right / top to bottom */
    uint8_t bottom_y[64], right_y[64];         /* row lcu_y + h - 1 and column lcu_x + w - 1 (w, h = LCU size inside the picture) */
    uint8_t bottom_cb[32], right_cb[32], bottom_cr[32], right_cr[32];
} SvtAmdLcuBorder;
SVT_AMD_API int svt_amd_encdec_picture_put_borders(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuBorder *borders, int n);
typedef struct SvtAmdLcuBorder16 {
    uint16_t lcu_x, lcu_y;
    uint8_t mode_bottom[16], mode_right[16];
    uint16_t bottom_y[64], right_y[64], bottom_cb[32], right_cb[32], bottom_cr[32], right_cr[32];
} SvtAmdLcuBorder16;
SVT_AMD_API int svt_amd_encdec_picture_put_borders16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdLcuBorder16 *borders, int n);

/* ------------------------------------------------------------------------- */
/* One transform unit of the final encode pass, end to end                     */
/* ------------------------------------------------------------------------- */
/* The product form of EncodeLoop + EncodeGenerateRecon (Codec/EbCodingLoop.c:651-1083, :1084-1243; 16-bit :1244-1797) for
 * one plane of one DCT unit with the default coefficient shape and no RDOQ / masking: PictureResidual -> EstimateTransform
 * -> UnifiedQuantizeInvQuantize -> EncodeInvTransform -> PictureAdditionKernel in ONE kernel, residual and coefficients in
 * registers.  Unit u: source block at d_src + src_off, prediction at d_rec + rec_off (overwritten by the reconstruction,
 * like the reference's in-place recon buffer); its quantised coefficients go to d_quant + u*size*size (row pitch = size),
 * the non-zero count to d_nz[u].  Bit depth 8 (1 byte per sample) or 10 (2 bytes). */
typedef struct SvtAmdEncodeUnit { int32_t src_off, rec_off; uint8_t qp, slice_type, pad[2]; uint32_t dz_offset; } SvtAmdEncodeUnit;
SVT_AMD_API int svt_amd_encode_tu_batch(SvtAmdContext *ctx, int bytes_per_sample, int size, const SvtAmdEncodeUnit *d_units,
                                        const void *d_src, uint32_t srcStride, void *d_rec, uint32_t recStride,
                                        int16_t *d_quant, uint32_t *d_nz, uint32_t nunits);

/* ------------------------------------------------------------------------- */
/* Quantiser of the final encode pass                                          */
/* ------------------------------------------------------------------------- */
/* Replaces UnifiedQuantizeInvQuantize (Codec/EbTransforms.c:2978-3250, called from EncodeLoop / EncodeLoop16bit,
 * Codec/EbCodingLoop.c:740-954, :1333-1550) on its paths without RDOQ / PM-core and without perceptual masking
 * (pmpMaskingLevelEncDec == 0; masking needs -brr 1): scaling constants from qp / bit depth / size / slice type
 * (:3097-3112), dead-zone override dZoffset (:3118), the DC-only shape (:3043-3090), the (size >> shape) active area,
 * the isolated-coefficient clean-up (:3190-3232) and UpdateQiQCoef (C_DEFAULT/EbTransforms_C.c:209) with the contouring
 * and forced-cbf flags.  Unit u: coefficients at d_coeff + u*1024 (row pitch = size); quantised / reconstructed
 * coefficients are written in the same layout (only the active area is touched), non-zero count to d_nz[u]. */
typedef struct SvtAmdQuantUnit {
    uint8_t  size;              /* 4 / 8 / 16 / 32                                                         */
    uint8_t  qp, bit_depth;     /* 8 or 10                                                                 */
    uint8_t  slice_type;        /* EB_PICTURE: 0 B, 1 P, 2 I, 3 IDR                                        */
    uint8_t  shape;             /* transCoeffShape: 0 default, 1 N2, 2 N4, 3 only DC                       */
    uint8_t  clean_sparse, enable_cb_flag, contouring_flag;
    uint8_t  component;         /* COMPONENT_LUMA 0, chroma otherwise                                      */
    uint8_t  temporal_layer;
    uint8_t  pad[2];
    uint32_t dz_offset;
} SvtAmdQuantUnit;
SVT_AMD_API int svt_amd_unified_quantize_batch(SvtAmdContext *ctx, const SvtAmdQuantUnit *d_units, const int16_t *d_coeff,
                                               int16_t *d_quant, int16_t *d_recon, uint32_t *d_nz, uint32_t nunits);
/* Per-call form on HOST pointers (row pitch coeffStride for all three blocks); blocking. */
SVT_AMD_API int svt_amd_unified_quantize(SvtAmdContext *ctx, const SvtAmdQuantUnit *unit, const int16_t *coeff,
                                         uint32_t coeffStride, int16_t *quant, int16_t *recon, uint32_t *nz);
/* The same reference function when contextPtr->mdContext->rdoqPmCoreMethod == EB_PMCORE (encMode 1..4; Codec/EbTransforms.c:
 * 3009-3052 -> DecoupledQuantizeInvQuantizeLoops :2605-2973): whole unit, no shapes / dead-zone override / clean-ups; luma units
 * get every 4x4 block of levels re-decided among 100 / 70 / 50 % coefficient scalings by SSE + lambda * rate (rate tables =
 * the CabacCost_t the call receives, `cost` is a HOST pointer), chroma units the plain quantiser. */
typedef struct SvtAmdPmQuantUnit {
    uint8_t  size;              /* 4 / 8 / 16 / 32                                                         */
    uint8_t  qp, bit_depth;     /* 8 or 10                                                                 */
    uint8_t  slice_type;        /* EB_PICTURE: 0 B, 1 P, 2 I, 3 IDR                                        */
    uint8_t  component;         /* COMPONENT_LUMA 0, chroma otherwise                                      */
    uint8_t  cand_type;         /* the `type` argument: INTER_MODE 1 / INTRA_MODE 2                        */
    uint8_t  pad[2];
    uint32_t lambda;            /* the `lambda` argument (contextPtr->fullLambda)                          */
} SvtAmdPmQuantUnit;
SVT_AMD_API int svt_amd_pmcore_quantize_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdPmQuantUnit *d_units,
                                              const int16_t *d_coeff, int16_t *d_quant, int16_t *d_recon, uint32_t *d_nz,
                                              uint32_t nunits);
SVT_AMD_API int svt_amd_pmcore_quantize(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdPmQuantUnit *unit,
                                        const int16_t *coeff, uint32_t coeffStride, int16_t *quant, int16_t *recon, uint32_t *nz);

/* ------------------------------------------------------------------------- */
/* Reconstruction of transform units (final encode pass)                      */
/* ------------------------------------------------------------------------- */
/* Replaces, per reconstructed plane of a transform unit, EncodeGenerateRecon / EncodeGenerateRecon16bit
 * (Codec/EbCodingLoop.c:1084-1243, :1660-1797; reached through the global table EncodeGenerateReconFunctionPtr, :1807):
 * EncodeInvTransform (Codec/EbTransforms.c:3502: DC-only shortcut, inverse DCT, inverse DST for the 4x4 luma unit) +
 * PictureAdditionKernel(16bit).  Unit u has its size x size inverse-quantised coefficients at d_coeff + u*size*size;
 * pred_off / recon_off = sample index of the unit's (0,0) in the prediction / reconstruction plane (the reference
 * reconstructs in place: both planes may be the same buffer with equal offsets). */
typedef struct SvtAmdReconUnit { int32_t pred_off, recon_off; uint8_t only_dc, dst, pad[2]; } SvtAmdReconUnit;
SVT_AMD_API int svt_amd_recon_tu_batch(SvtAmdContext *ctx, int bytes_per_sample, int size, const int16_t *d_coeff,
                                       const SvtAmdReconUnit *d_units, const void *d_pred, uint32_t predStride,
                                       void *d_recon, uint32_t reconStride, uint32_t nunits);
/* Per-call form on HOST pointers (strides in samples; coeffStride 64 / 32 for the reference's LCU scratch planes).
 * Blocking; used by the EncodeGenerateReconFunctionPtr binding. */
SVT_AMD_API int svt_amd_recon_tu(SvtAmdContext *ctx, int bytes_per_sample, int size, int only_dc, int dst,
                                 const int16_t *coeff, uint32_t coeffStride, const void *pred, uint32_t predStride,
                                 void *recon, uint32_t reconStride);

/* ------------------------------------------------------------------------- */
/* Chroma full loop of one mode-decision candidate                            */
/* ------------------------------------------------------------------------- */
/* Replaces the pair FullLoop_R (Codec/EbFullLoop.c:579-870) + CuFullDistortionFastTuMode_R (:873-1066) as the mode
 * decision calls them with PICTURE_BUFFER_DESC_CHROMA_MASK (EbProductCodingLoop.c:4291-4319 and :4518-4547), for the same
 * configuration as the luma loop above (no RDOQ / PM-core, coefficient-domain distortion, no CABAC-context update).
 * Per chroma transform unit (size/2, four 16x16 for a 64x64 CU) and plane: EstimateTransform (EbTransforms.c:3268) ->
 * UnifiedQuantizeInvQuantize_R (EbFullLoop.c:452) -> PictureFullDistortion_R (EbPictureOperators.c:325) + the chroma
 * scaling (EbFullLoop.c:1000-1004) -> TuEstimateCoeffBits_R (EbEntropyCoding.c:7963) -> TuCalcCost chroma branches
 * (EbRateDistortionCost.c:273-279).  Partial-frequency correction as :647-652 (4x4 never, 8x8 at most N2). */
typedef struct SvtAmdChromaLoopIn {
    uint32_t size;              /* CU size 8 / 16 / 32 / 64 (chroma TU = size/2, 16 for 64)              */
    uint32_t cb_qp, cr_qp;      /* MapChromaQp() outputs the caller derived                              */
    uint32_t slice_type;        /* EB_PICTURE: 0 B, 1 P, 2 I, 3 IDR                                      */
    uint32_t pf_mode;           /* contextPtr->pfMdMode: 0 off, 1 N2                                     */
    uint32_t cand_type;         /* INTER_MODE 1 / INTRA_MODE 2                                           */
    uint32_t intra_luma_mode;   /* chroma mode is EB_INTRA_CHROMA_DM in this loop                        */
    uint32_t pad;
} SvtAmdChromaLoopIn;
typedef struct SvtAmdChromaLoopOut {
    uint32_t nz[2][5];          /* countNonZeroCoeffs[1 / 2][0..4] entries the call wrote (others 0)     */
    uint32_t cbf[2];            /* candidatePtr->cbCbf / crCbf (zeroed by the caller between the two)    */
    uint64_t coeff_bits[2];     /* *cbCoeffBits / *crCoeffBits (the caller passes zeros in)              */
    uint64_t dist[2][2];        /* cb / cr FullDistortion[DIST_CALC_RESIDUAL / PREDICTION]               */
} SvtAmdChromaLoopOut;
/* BATCHED: candidate c has its (size/2)^2 Cb residual at d_residual + c*2048 and its Cr residual 1024 samples later
 * (row pitch = size/2); quantised and reconstructed coefficients come back in the same layout. `cost`: HOST pointer. */
SVT_AMD_API int svt_amd_full_loop_chroma_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost,
                                               const SvtAmdChromaLoopIn *d_in, const int16_t *d_residual,
                                               int16_t *d_quant, int16_t *d_recon, SvtAmdChromaLoopOut *d_out,
                                               uint32_t ncand);
/* Per-call form on HOST pointers ([0] = Cb, [1] = Cr; row pitch `pitch` samples, e.g. the reference's 32-sample chroma
 * LCU buffers); writes back only the (T >> pf) area of every transform unit.  Blocking. */
SVT_AMD_API int svt_amd_full_loop_chroma(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdChromaLoopIn *in,
                                         const int16_t *const residual[2], int16_t *const quant[2],
                                         int16_t *const recon[2], uint32_t pitch, SvtAmdChromaLoopOut *out);
/* coeffCabacUpdate forms (the mode decision of full-depth pictures: EbEncDecProcess.c:2115-2123; call sites EbFullLoop.c:265-280,
 * 417-432, 1014-1035): the coefficient bits of every unit come from the context-updating estimator and the candidate's
 * CoeffCtxtMdl_t (candidateBuffer->candBuffCoeffCtxModel; SVT_AMD_COEFF_CTX_WORDS words, see svt_amd_coeff_bits_update_batch) is
 * updated in place, unit after unit (chroma: Cb then Cr of every unit). */
SVT_AMD_API int svt_amd_full_loop_luma_cabac_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdFullLoopIn *d_in,
                                                   const int16_t *d_residual, int16_t *d_quant, int16_t *d_recon,
                                                   SvtAmdFullLoopOut *d_out, uint32_t *d_ctx_models, uint32_t ncand);
SVT_AMD_API int svt_amd_full_loop_chroma_cabac_batch(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdChromaLoopIn *d_in,
                                                     const int16_t *d_residual, int16_t *d_quant, int16_t *d_recon,
                                                     SvtAmdChromaLoopOut *d_out, uint32_t *d_ctx_models, uint32_t ncand);
SVT_AMD_API int svt_amd_full_loop_luma_cabac(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdFullLoopIn *in,
                                             const int16_t *residual, int16_t *quant, int16_t *recon, uint32_t pitch,
                                             uint32_t *ctx_model, SvtAmdFullLoopOut *out);
SVT_AMD_API int svt_amd_full_loop_chroma_cabac(SvtAmdContext *ctx, const SvtAmdCabacCost *cost, const SvtAmdChromaLoopIn *in,
                                               const int16_t *const residual[2], int16_t *const quant[2], int16_t *const recon[2],
                                               uint32_t pitch, uint32_t *ctx_model, SvtAmdChromaLoopOut *out);

/* ------------------------------------------------------------------------- */
/* HEVC motion-compensation interpolation (closed-loop inter prediction)      */
/* ------------------------------------------------------------------------- */
/* One prediction block: integer position = sample index ref_off of the reference plane, fractional part (fx,fy) in
 * quarter samples for luma (0..3), eighth samples for chroma (0..7); output at sample index dst_off.
 * Raw (int16, bi-prediction intermediate) output is packed with stride = w at dst_off.  w, h <= 64. */
typedef struct SvtAmdMcpBlock { int32_t ref_off, dst_off; uint16_t w, h; uint8_t fx, fy, pad[2]; } SvtAmdMcpBlock;
typedef struct SvtAmdBiPredBlock { int32_t l0_off, l1_off, dst_off; uint16_t w, h; } SvtAmdBiPredBlock;
/* BATCHED (device pointers): replaces the per-PU calls of UniPredHevcInterpolationMd / EncodeUniPredInterpolation
 * (Codec/EbMcp.c:99-600) into uniPredLumaIFFunctionPtrArrayNew / uniPredChromaIFFunctionPtrArrayNew (out_raw 0) and of
 * BiPredHevcInterpolationMd (:601-1016) into biPredLumaIFFunctionPtrArrayNew / biPredChromaIFFunctionPtrArrayNew
 * (out_raw 1) followed by biPredClippingFuncPtrArray (Codec/EbMcpTables.c:14-745). */
SVT_AMD_API int svt_amd_mcp_batch(SvtAmdContext *ctx, int bytes_per_sample, int chroma, int out_raw, const void *d_ref,
                                  uint32_t refStride, void *d_dst, uint32_t dstStride,
                                  const SvtAmdMcpBlock *d_blocks, uint32_t nblocks);
/* the same with a promise about the largest block width / height of the list (0 = unknown, up to 64): smaller blocks
 * need less LDS, so more of them are in flight per CU */
SVT_AMD_API int svt_amd_mcp_batch_sized(SvtAmdContext *ctx, int bytes_per_sample, int chroma, int out_raw, const void *d_ref,
                                        uint32_t refStride, void *d_dst, uint32_t dstStride,
                                        const SvtAmdMcpBlock *d_blocks, uint32_t nblocks, uint32_t max_block_dim);
/* offset: Offset5 (luma) / ChromaOffset5 of Codec/EbDefinitions.h:1022-1030; ignored for 16-bit */
SVT_AMD_API int svt_amd_bipred_clip_batch(SvtAmdContext *ctx, int bytes_per_sample, const int16_t *d_l0,
                                          const int16_t *d_l1, void *d_dst, uint32_t dstStride, int32_t offset,
                                          const SvtAmdBiPredBlock *d_blocks, uint32_t nblocks);

/* LEAF forms: the distinct C_DEFAULT symbols of uniPredLumaIFFunctionPtrArrayNew[16], biPredLumaIFFunctionPtrArrayNew[16],
 * uniPredChromaIFFunctionPtrArrayNew[64], biPredChromaIFFunctionPtrArrayNew[64], their 16-bit twins and the two
 * clipping tables.  firstPassIFDst is the reference's scratch buffer; it is not written. */
#define SVT_AMD_DECL_MCP_UNI(name, T)                                                                          \
    SVT_AMD_API void svt_amd_##name(T *refPic, uint32_t srcStride, T *dst, uint32_t dstStride, uint32_t puWidth, \
                                    uint32_t puHeight, int16_t *firstPassIFDst);
#define SVT_AMD_DECL_MCP_RAW(name, T)                                                                          \
    SVT_AMD_API void svt_amd_##name(T *refPic, uint32_t srcStride, int16_t *dst, uint32_t puWidth,             \
                                    uint32_t puHeight, int16_t *firstPassIFDst);
#define SVT_AMD_DECL_MCP_CUNI(name, T)                                                                         \
    SVT_AMD_API void svt_amd_##name(T *refPic, uint32_t srcStride, T *dst, uint32_t dstStride, uint32_t puWidth, \
                                    uint32_t puHeight, int16_t *firstPassIFDst, uint32_t fracPosx, uint32_t fracPosy);
#define SVT_AMD_DECL_MCP_CRAW(name, T)                                                                         \
    SVT_AMD_API void svt_amd_##name(T *refPic, uint32_t srcStride, int16_t *dst, uint32_t puWidth,             \
                                    uint32_t puHeight, int16_t *firstPassIFDst, uint32_t fracPosx, uint32_t fracPosy);
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosaNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosaNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosaOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosaOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosbNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosbNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosbOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosbOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoscNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoscNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoscOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoscOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosdNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosdNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosdOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosdOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoseNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoseNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoseOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoseOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosfNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosfNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosfOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosfOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosgNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosgNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosgOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosgOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoshNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoshNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoshOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoshOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosiNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosiNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosiOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosiOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosjNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosjNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosjOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosjOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoskNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPoskNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoskOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPoskOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosnNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosnNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosnOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosnOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPospNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPospNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPospOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPospOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosqNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosqNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosqOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosqOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosrNew, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationFilterPosrNew16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosrOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationFilterPosrOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationCopy, uint8_t)
SVT_AMD_DECL_MCP_UNI(LumaInterpolationCopy16bit, uint16_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationCopyOutRaw, uint8_t)
SVT_AMD_DECL_MCP_RAW(LumaInterpolationCopyOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_CUNI(ChromaInterpolationCopy, uint8_t)
SVT_AMD_DECL_MCP_CUNI(ChromaInterpolationFilterOneD, uint8_t)
SVT_AMD_DECL_MCP_CUNI(ChromaInterpolationFilterTwoD, uint8_t)
SVT_AMD_DECL_MCP_CUNI(ChromaInterpolationCopy16bit, uint16_t)
SVT_AMD_DECL_MCP_CUNI(ChromaInterpolationFilterOneD16bit, uint16_t)
SVT_AMD_DECL_MCP_CUNI(ChromaInterpolationFilterTwoD16bit, uint16_t)
SVT_AMD_DECL_MCP_CRAW(ChromaInterpolationCopyOutRaw, uint8_t)
SVT_AMD_DECL_MCP_CRAW(ChromaInterpolationFilterOneDOutRaw, uint8_t)
SVT_AMD_DECL_MCP_CRAW(ChromaInterpolationFilterTwoDOutRaw, uint8_t)
SVT_AMD_DECL_MCP_CRAW(ChromaInterpolationCopyOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_CRAW(ChromaInterpolationFilterOneDOutRaw16bit, uint16_t)
SVT_AMD_DECL_MCP_CRAW(ChromaInterpolationFilterTwoDOutRaw16bit, uint16_t)
SVT_AMD_API void svt_amd_BiPredClipping(uint32_t puWidth, uint32_t puHeight, int16_t *list0Src, int16_t *list1Src,
                                        uint8_t *dst, uint32_t dstStride, int32_t offset);
SVT_AMD_API void svt_amd_BiPredClipping16bit(uint32_t puWidth, uint32_t puHeight, int16_t *list0Src, int16_t *list1Src,
                                             uint16_t *dst, uint32_t dstStride);


/* ------------------------------------------------------------------------- */
/* Device-resident mode decision: ModeDecisionLcu + EncodePass of whole pictures */
/* ------------------------------------------------------------------------- */
/* The closed loop of an LCU on the device (SURVEY 8a rows ModeDecisionLcu / ProductPerformFastLoop / PerformFullLoop / inter-depth
 * decision + the EncDec input contract): ONE call per picture replaces, for every LCU, what EncDecKernel's LCU loop does between
 * ModeDecisionConfigureLcu and the end of EncodePass (Codec/EbEncDecProcess.c:2893-3023):
 *   ModeDecisionLcu (Codec/EbProductCodingLoop.c:4691-5114): the coding-unit loop over the LCU's MdcLcuData_t leaf list - context
 *   generation, candidate injection (Codec/EbModeDecision.c:1795), the two fast loops (:1911; prediction + NxM SAD + fast cost,
 *   Codec/EbRateDistortionCost.c:440), PreModeDecision (EbModeDecision.c:300), the full loop of the surviving candidates (:4351;
 *   ProductFullLoop, Codec/EbFullLoop.c:185, + the full-cost function, EbRateDistortionCost.c:963), ProductFullModeDecision
 *   (EbModeDecision.c:1995), the candidate's reconstruction (PerformInverseTransformRecon, :1334), the inter-depth decision
 *   (EbFullLoop.c:1461) and the neighbour-array updates (:371) - followed by the LCU's EncodePass (the encode unit above) on the tree
 *   it decided, and the wavefront of AssignEncDecSegments over the picture, all in one launch.
 * The mode decision's neighbour arrays (pcs->md*NeighborArray[MD_NEIGHBOR_ARRAY_INDEX], EbPictureControlSet.h) live in HBM as
 * picture-sized maps of the SvtAmdEncDecPicture (candidate reconstruction, mode type, intra luma mode, depth, skip flag), the
 * ME / OIS results are read where the front half left them.
 *
 * THIS REVISION covers the pictures whose LCUs all take the ModeDecisionLcu path with luma-only candidates (chroma level 1,
 * CHROMA_MODE_BEST: no chroma in the mode decision, EbEncDecProcess.c:2056-2113), no CABAC-context update, intra 4x4 off, plain
 * quantiser, no delta-QP tools, 8-bit:
 *   I pictures (PICT_FULL84_DEPTH_MODE), closed-loop intra (intraMdOpenLoopFlag == 0) = the I pictures of encMode 8..10 at every
 *   resolution and of encMode 7 in 4K (BASELINE configs[0], and the I pictures of configs[1] / [2] / [3]);
 *   P / B pictures (SvtAmdMdInter below) with open-loop intra candidates, with or - 8-bit pictures only - without sub-sample search
 *   (use_subpel 0: the candidates of the motion estimation rounded to whole samples, the merge candidates predicted at the rounded
 *   position, prediction through the reference's interpolation-free path), unrestricted motion vectors, the AMVP
 *   table generated in the mode decision and partial-frequency level 0 / 1 whose LCUs are all decided by ModeDecisionLcu (no
 *   branch-and-depth-pillar LCUs) = the non-reference B pictures of encMode 7..8 (half the pictures of a random-access encode).
 * svt_amd_md_picture_supported() says so; everything else stays with the reference code.
 * The controls below are DERIVED BY THE REFERENCE'S HOST CODE (SignalDerivationEncDecKernelOq, ProductResetModeDecision,
 * ModeDecisionConfigureLcu, the picture-analysis detectors) and are inputs here, like SvtAmdMeParams. */
typedef struct SvtAmdMdRates {             /* MdRateEstimationContext_t, field for field (Codec/EbMdRateEstimation.h:113-161)      */
    uint32_t splitFlagBits[6], skipFlagBits[6], mvpIndexBits[2], intraPartSizeBits[2], interPartSizeBits[8], predModeBits[2];
    uint32_t intraLumaBits[4], intraChromaBits[5], refPicBits[3], mvdBits[12], lumaCbfBits[10], chromaCbfBits[10], rootCbfBits[2];
    uint32_t transSubDivFlagBits[6], mergeFlagBits[2], mergeIndexBits[5], saoMergeFlagBits[2], saoTypeIndexBits[6];
    uint32_t saoOffsetTrunUnaryBits[8], interBiDirBits[8], interUniDirBits[2], pad[17];
} SvtAmdMdRates;
typedef struct SvtAmdMdPicture {
    uint16_t width, height;                /* luma                                                                               */
    uint8_t slice_type;                    /* EB_PICTURE: 0 B, 1 P, 2 I                                                          */
    uint8_t temporal_layer, is_reference, enc_mode;
    uint8_t depth_mode;                    /* ppcs->depthMode (PICT_FULL85 1, PICT_FULL84 2, ... EbDefinitions.h)                */
    uint8_t intra_md_open_loop;            /* ModeDecisionContext_t.intraMdOpenLoopFlag                                          */
    uint8_t intra_injection_method;        /* .intraInjectionMethod (EbEncDecProcess.c:2014-2026)                                */
    uint8_t limit_intra;                   /* .limitIntra                                                                        */
    uint8_t mpm_search, mpm_search_candidate; /* ConfigureMpm (Codec/EbModeDecisionProcess.c:560)                                */
    uint8_t pf_md_level, nfl_level_md, nmm_level_md;
    uint8_t full_loop_escape, single_fast_loop, coeff_cabac_update, spatial_sse_full_loop;
    uint8_t chroma_level;                  /* .chromaLevel                                                                       */
    uint8_t intra4x4_level;                /* .intra4x4Level (2 = off)                                                           */
    uint8_t rdoq_pmcore_method;            /* .rdoqPmCoreMethod (0 = plain quantiser)                                            */
    uint8_t skip_ois_8x8, cu8x8_mode, cu16x16_mode, limit_ois_to_dc_mode; /* PictureParentControlSet_t                            */
    uint8_t constrained_intra, strong_smoothing; /* encode pass: pcs->constrainedIntraFlag, scs->enableStrongIntraSmoothing      */
    uint8_t qp, chroma_qp;                 /* contextPtr->qp, ->chromaQp of every LCU (no delta-QP tools)                        */
    uint8_t intra8x8_restriction_inter_slice; /* .intra8x8RestrictionInterSlice (EbEncDecProcess.c:2125-2151)                    */
    uint8_t pad;
    uint32_t fast_lambda, full_lambda, fast_chroma_lambda, full_chroma_lambda; /* ModeDecisionConfigureLcu's assignment           */
    SvtAmdMdRates rates;                   /* contextPtr->mdRateEstimationPtr (slice type + QP row of mdRateEstimationArray)     */
} SvtAmdMdPicture;
#define SVT_AMD_MD_LEAVES 85               /* CU_MAX_COUNT                                                                       */
typedef struct SvtAmdMdLcu {
    uint8_t leaf_count;                    /* MdcLcuData_t.leafCount, .leafDataArray[] (EbPictureControlSet.h:82-102)            */
    uint8_t leaf_index[SVT_AMD_MD_LEAVES], leaf_split[SVT_AMD_MD_LEAVES];
    uint8_t tile_left, tile_top, tile_right; /* lcuEdgeInfoPtr                                                                   */
    uint8_t is_complete;                   /* scs->lcuParamsArray[lcu].isCompleteLcu                                             */
    uint8_t complexity_status_2;           /* ppcs->complexLcuArray[lcu] == LCU_COMPLEXITY_STATUS_2                              */
    uint8_t contouring_class[4];           /* DeriveContouringClass of the four 32x32 quadrants (EbModeDecisionConfiguration.c:395) */
    uint8_t chroma_encode_mode;            /* lcuPtr->chromaEncodeMode after ConfigureChroma (1 = CHROMA_MODE_FULL, 2 = CHROMA_MODE_BEST)             */
    uint8_t restrict_intra_global_motion;  /* contextPtr->restrictIntraGlobalMotion                                              */
    uint8_t lcu_md_mode;                   /* ppcs->lcuMdModeArray[lcu] (PICT_LCU_SWITCH pictures)                               */
    uint8_t skip_small_cu;                 /* SkipSmallCu's LCU condition (EbProductCodingLoop.c:2301): auraStatus == AURA_STATUS_0 and no
                                            * stationary edge over time                                                          */
    uint8_t cmplx_noise;                   /* ppcs->cmplxStatusLcu[lcu] == CMPLX_NOISE (:2079)                                   */
    uint8_t variance_below_200;            /* ppcs->variance[lcu][0] < 200: the encode pass's skip-cost bias (EbCodingLoop.c:3866) */
    uint8_t edge_block;                    /* ppcs->edgeResultsPtr[lcu].edgeBlockNum != 0                                        */
    uint8_t no_stop_split;                 /* StopSplitCondition's LCU exemptions (Codec/EbFullLoop.c:1445-1450): isolated non-homogeneous
                                            * area, or aura status 1 below 4K                                                    */
    uint8_t pad[3];
} SvtAmdMdLcu;
/* P / B pictures: what the inter candidates need beyond the above.  Reference pictures and coefficient-rate tables are those of
 * svt_amd_encdec_picture_set_inter (the mode decision predicts from the same reference pictures as the encode pass). */
typedef struct SvtAmdTmvpLcu {             /* TmvpUnit_t of one LCU (Codec/EbAdaptiveMotionVectorPrediction.h:28): 16 units of 16x16 */
    int16_t mv[2][16][2];                  /* [list][unit]{x, y}                                                                 */
    uint64_t ref_poc[2][16];
    uint8_t pred_dir[16], available[16];
} SvtAmdTmvpLcu;
typedef struct SvtAmdMdInter {
    uint64_t picture_number;               /* pcs->pictureNumber                                                                 */
    uint64_t ref_poc[2];                   /* ((EbReferenceObject_t *)pcs->refPicPtrArray[list]->objectPtr)->refPOC              */
    uint64_t colocated_poc;                /* refPOC of the co-located picture (list pcs->colocatedPuRefList; list 0 in P pictures) */
    uint8_t colocated_pu_ref_list, is_low_delay; /* pcs->colocatedPuRefList, ->isLowDelay                                        */
    uint8_t tmvp_enable;                   /* !ppcs->disableTmvpFlag && the co-located reference object's tmvpEnableFlag         */
    uint8_t use_subpel;                    /* ppcs->useSubpelFlag (0: encMode 9 at the 4K input class, layers above 0; 8-bit calls) */
    uint8_t unrestricted_mv;               /* scs->staticConfig.unrestrictedMotionVector                                         */
    uint8_t generate_amvp_table_md;        /* ModeDecisionContext_t.generateAmvpTableMd                                          */
    uint8_t extra_injection;               /* .amvpInjection | .unipred3x3Injection | .bipred3x3Injection (encMode 0..1)         */
    uint8_t improve_sharpness;             /* scs->staticConfig.improveSharpness (cost biases)                                   */
    uint8_t skip_cost_bias;                /* encode pass (EbCodingLoop.c:3861-3871): non-reference B picture with a reference picture whose
                                            * intraCodedArea is above INTRA_AREA_TH[its temporal layer]                          */
    uint8_t pad[3];
    uint32_t chroma_weight;                /* ChromaWeightFactor*[qp] of the picture's class (Codec/EbRateDistortionCost.c:35-65, EbLambdaRateTables.h): the weight
                                            * of chroma distortion in the merge / skip costs                                       */
} SvtAmdMdInter;
/* what the mode decision leaves per LCU: the decision of every leaf it tested (the final tree = leaves with split == 0 walked in
 * Z order) and the costs the inter-depth decisions compared (mdLocalCuUnit[].cost) */
typedef struct SvtAmdMdLcuOut {
    uint8_t split[SVT_AMD_MD_LEAVES];      /* CodingUnit_t.splitFlag after the call                                              */
    uint8_t tested[SVT_AMD_MD_LEAVES];     /* mdLocalCuUnit[].testedCuFlag                                                       */
    uint8_t pred_mode[SVT_AMD_MD_LEAVES];  /* predictionModeFlag of tested leaves                                                */
    uint8_t intra_luma_mode[SVT_AMD_MD_LEAVES];
    uint8_t ycbf[SVT_AMD_MD_LEAVES];       /* luma cbf as ProductFullModeDecision left it: bit 0 = transformUnitArray[0].lumaCbf (units below
                                            * 64x64), bits 1..4 = transform units 1..4 of a 64x64 unit                           */
    uint8_t inter_dir[SVT_AMD_MD_LEAVES];  /* PredictionUnit_t.interPredDirectionIndex (3 in intra units)                        */
    uint8_t merge_flag[SVT_AMD_MD_LEAVES], merge_index[SVT_AMD_MD_LEAVES];
    uint8_t pad[8];
    int16_t mv[SVT_AMD_MD_LEAVES][2][2];   /* PredictionUnit_t.mv[list].{x, y}                                                   */
    uint64_t cost[SVT_AMD_MD_LEAVES];      /* mdLocalCuUnit[].cost                                                               */
    uint64_t merge_cost[SVT_AMD_MD_LEAVES], skip_cost[SVT_AMD_MD_LEAVES]; /* mdEpPipeLcu[].mergeCost / .skipCost (merge units)   */
} SvtAmdMdLcuOut;
/* 1 when this revision's device call covers the picture (see above) */
SVT_AMD_API int svt_amd_md_picture_supported(const SvtAmdMdPicture *P);
/* The whole picture: mode decision + encode pass of every LCU, one launch, wavefront on the device.  HOST arrays of every LCU in
 * raster order: lcus (controls) in; md_out (decisions), works (the EncDec input contract the decisions amount to, source samples
 * included) and results (the encode pass's output contract) out - any of the three may be NULL.  src_y / src_cb / src_cr: HOST
 * planes of the picture's source (enhancedPicturePtr), sample (0,0), strides in samples.  ois: HOST array of the picture's
 * open-loop intra search results, or NULL - then the records svt_amd_ois_picture* left in HBM for `ois_slot` are read.  cost: the
 * picture's coefficient-rate tables (pcs->cabacCost).  Blocking.
 * Source planes with rows contiguous in memory (stride_y < 2 * width + 256, multiples of 4) travel as ONE linear transfer each: the call then READS the
 * caller's inter-row padding too - stride * (rows - 1) + width bytes from src_y / src_cb / src_cr must be readable (an encoder's padded picture buffer is;
 * a plane assembled from separately allocated rows must be passed with a stride that fails the test, or copied first).
 * Round 6: the call is two kernels on the context's stream - the decisions of every LCU (wavefront on the device), then the encode pass of every LCU from the work
 * records the first left in HBM.
 * lcus == NULL: the controls are the DEVICE array svt_amd_md_picture_set_controls bound to `pic` for this call - read in place, no upload, no host loop over
 * the LCUs; without a binding the call is refused as before. */
SVT_AMD_API int svt_amd_md_encode_picture(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus,
                                          const uint8_t *src_y, uint32_t stride_y, const uint8_t *src_cb, const uint8_t *src_cr,
                                          uint32_t stride_c, const SvtAmdOisLcuResult *ois, int ois_slot, const SvtAmdCabacCost *cost,
                                          SvtAmdMdLcuOut *md_out, SvtAmdLcuWork *works, SvtAmdLcuResult *results);
/* P / B pictures: the same call with the inter inputs - X (above), me: HOST array of the picture's motion-estimation results (one
 * record per LCU; NULL = the records svt_amd_me_picture* left in HBM for `me_slot`), tmvp: HOST array of the co-located picture's
 * motion field (one record per LCU; may be NULL when !X->tmvp_enable).  The reference pictures and rate tables are those of the
 * last svt_amd_encdec_picture_set_inter on `pic`.  X == NULL: an I picture, as above. */
SVT_AMD_API int svt_amd_md_encode_picture_inter(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdInter *X,
                                                const SvtAmdMdLcu *lcus, const uint8_t *src_y, uint32_t stride_y, const uint8_t *src_cb,
                                                const uint8_t *src_cr, uint32_t stride_c, const SvtAmdOisLcuResult *ois, int ois_slot,
                                                const SvtAmdMeLcuResult *me, int me_slot, const SvtAmdTmvpLcu *tmvp,
                                                SvtAmdMdLcuOut *md_out, SvtAmdLcuWork *works, SvtAmdLcuResult *results);
/* The same two calls for a 10-bit picture (a picture object created with bytes_per_sample = 2; encoderBitDepth 10, BASELINE configs[3]).  The reference's mode decision
 * stays an 8-bit process there - its source is the input picture's 8-bit plane, its inter candidates are predicted from the 8 most significant bits of the 16-bit reference
 * pictures (Inter2Nx2NPuPredictionHevc with is16bit: UnPackReferenceBlock, Codec/EbInterPrediction.c:414-457, :589-760; AddChromaEncDec likewise, EbCodingLoop.c:3841) - and
 * only EncodePass codes the 10-bit samples (EncodePassPackLcu, EbCodingLoop.c:2867).  src_*: HOST planes of the 10-bit source in 16-bit words (8-bit plane << 2 | the two
 * extra bits), strides in samples; the call derives the 8-MSB views of the source and of the picture object's 16-bit reference pictures on the device and decides on
 * those, then encodes on the 10-bit samples: works / results are the 16-bit records of svt_amd_encode_picture16.  Decisions (md_out) as in the 8-bit calls. */
SVT_AMD_API int svt_amd_md_encode_picture16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus,
                                            const uint16_t *src_y, uint32_t stride_y, const uint16_t *src_cb, const uint16_t *src_cr,
                                            uint32_t stride_c, const SvtAmdOisLcuResult *ois, int ois_slot, const SvtAmdCabacCost *cost,
                                            SvtAmdMdLcuOut *md_out, SvtAmdLcuWork16 *works, SvtAmdLcuResult16 *results);
SVT_AMD_API int svt_amd_md_encode_picture_inter16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdInter *X,
                                                  const SvtAmdMdLcu *lcus, const uint16_t *src_y, uint32_t stride_y, const uint16_t *src_cb,
                                                  const uint16_t *src_cr, uint32_t stride_c, const SvtAmdOisLcuResult *ois, int ois_slot,
                                                  const SvtAmdMeLcuResult *me, int me_slot, const SvtAmdTmvpLcu *tmvp, SvtAmdMdLcuOut *md_out,
                                                  SvtAmdLcuWork16 *works, SvtAmdLcuResult16 *results);
SVT_AMD_API int svt_amd_md_picture_supported_inter(const SvtAmdMdPicture *P, const SvtAmdMdInter *X);
/* ... by the 16-bit entry (svt_amd_md_encode_picture_inter16, the launch on a 16-bit picture object): the same pictures except those coded without sub-sample search
 * (use_subpel 0), whose prediction from 10-bit reference pictures (UnpackUniPredRef10Bit / UnpackBiPredRef10Bit) is a path of its own this revision does not hold */
SVT_AMD_API int svt_amd_md_picture_supported_inter16(const SvtAmdMdPicture *P, const SvtAmdMdInter *X);
/* 1 when every one of the n LCUs is decided by ModeDecisionLcu with luma-only candidates (the per-LCU half of the two checks above) */
SVT_AMD_API int svt_amd_md_lcus_supported(const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus, int n);
/* Binds a DEVICE array of the picture object's LCU count (svt_amd_md_controls_batch_launch's output, or any array of that layout) as the controls of the NEXT
 * svt_amd_md_encode_picture[_inter][16] call on `pic`, and of that call only: the call consumes the binding whether it succeeds or refuses.  That call must pass
 * lcus == NULL; one that passes host lcus as well is refused and drops the binding.  d_lcus == NULL drops a binding.  The array must stay valid until the blocking
 * call returns.  Written on the context the call runs on, stream order suffices; written on another lane, ordering it is the caller's
 * (svt_amd_lane_event_record / _wait), as for every raw device pointer here.  The call then runs a check kernel over the array first (SvtAmdMdCtlCheck above), copies
 * that one record to the host and synchronises once, refuses what the host loop refuses - in the same words, naming the first offending LCU - and points the
 * mode-decision kernel at the array.  A picture object with a rank rectangle (svt_amd_encdec_picture_set_rect) is refused with a bound array: the tile-border check
 * of that path reads host records. */
SVT_AMD_API int svt_amd_md_picture_set_controls(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdLcu *d_lcus);

/* The same picture call as a STREAM-ORDERED LAUNCH on DEVICE inputs: mode decision and encode pass of one picture queued on ctx's stream, then the call returns.
 * It synchronises nothing, copies nothing from or to host memory and waits for no event; it allocates only at the first call on the picture object (and, for the
 * check record, on the context).  The decisions, work records and results stay in HBM, where svt_amd_encdec_picture_tail_launch (NULL records) and
 * svt_amd_encdec_picture_motion_field read them in place - queued behind this call on the same context, stream order suffices - and
 * svt_amd_encdec_picture_md_records hands them out.  The blocking entries above are unchanged; both kinds may alternate on one object.
 *   P, X, cost   HOST records, read before the call returns (they travel in a kernel-argument block, so a second launch on the same object queued before the first
 *                has run cannot disturb the first).  X == NULL: an I picture.  cost == NULL keeps the rate tables svt_amd_encdec_picture_set_inter put on the
 *                object; required when the object has none.
 *   d_lcus       DEVICE SvtAmdMdLcu[LCUs] (svt_amd_md_controls_batch_launch's output, or any array of that layout), required.
 *   d_src        DEVICE source planes of the object's sample width (8-bit samples, or 10-bit samples in 16-bit words), sample (0,0); pitches in samples.
 *                Pointers and row starts 4-byte aligned: pitch >= plane width, pitch * bytes per sample a multiple of 4.  The planes are COPIED into the object's
 *                own (for 16-bit samples the 8-MSB view is made in the same pass): the caller may reuse them once the launch has run.
 *   d_ois, d_me  DEVICE arrays of one record per LCU read in place, or NULL: the records resident in picture slot ois_slot / me_slot - the stream orders itself
 *                behind the launch that wrote them and leaves a read mark, exactly as the blocking call does.  d_me and me_slot are ignored for an I picture.
 *   d_tmvp       DEVICE SvtAmdTmvpLcu[LCUs + 1] (svt_amd_encdec_picture_motion_field's output), 8-byte aligned: required when X->tmvp_enable, ignored otherwise.
 *   tiles        the picture's tile count (LCUs with tile_left && tile_top), 1 .. LCUs: it sizes the grids only - a wrong count costs time, never correctness.
 *   flags        SVT_AMD_MD_LAUNCH_DECIDE_ONLY: a P / B picture's decisions alone - no work records, no encode pass (the blocking call with works == results == NULL).
 * Every raw device pointer is the caller's to order: written on this context, stream order suffices; written on another lane, svt_amd_lane_event_record / _wait.
 * Everything the host can judge is checked before anything is queued - svt_amd_md_picture_supported[_inter], the picture object's size and sample width,
 * reference pictures and rate tables, complete slot records, pitches and alignment, pads and flags; an object with a rank rectangle
 * (svt_amd_encdec_picture_set_rect) is refused, and so is a call that finds a binding of svt_amd_md_picture_set_controls / _set_motion_field pending on the object,
 * which it drops: the job carries the arrays.  A refusal names this entry and queues nothing.
 * What the blocking call's host loop refuses in the CONTROLS (SvtAmdMdCtlCheck: leaf_count, leaf list, an LCU not decided by ModeDecisionLcu in a P / B picture) is
 * judged on the device: the check kernel runs over d_lcus, and for an array it refuses nothing of the picture is decided or encoded - no LCU of a malformed leaf
 * list is read, d_out keeps what it held, work and result records are zero (the tail counts every such LCU but the first - a zero record is an empty LCU at (0, 0) - in
 * SvtAmdTailCheck.bad_lcus, the motion field reads them as empty).  d_status (DEVICE, 4-byte aligned, or NULL) receives that check record and `refused` once per launch.
 * Launch width: the blocking call's formulas; a launch cannot wait for the workgroup budget of the blocking calls and holds none of it - it takes the lone
 * picture's width when no blocking call is in flight as it is queued and the narrow one otherwise.  Tickets make any width correct.
 * The object's debug profile / trace switches apply as in the blocking call; SVT_AMD_MD_TIMING does not. */
#define SVT_AMD_MD_LAUNCH_DECIDE_ONLY 1u
typedef struct SvtAmdMdLaunchJob {
    const SvtAmdMdPicture *P;              /* HOST                                                                               */
    const SvtAmdMdInter *X;                /* HOST, or NULL: an I picture                                                        */
    const SvtAmdCabacCost *cost;           /* HOST, or NULL: the object's rate tables                                            */
    const SvtAmdMdLcu *d_lcus;             /* DEVICE                                                                             */
    const void *d_src[3];                  /* DEVICE: luma, cb, cr                                                               */
    const SvtAmdOisLcuResult *d_ois;       /* DEVICE, or NULL: slot ois_slot                                                     */
    const SvtAmdMeLcuResult *d_me;         /* DEVICE, or NULL: slot me_slot (P / B)                                              */
    const SvtAmdTmvpLcu *d_tmvp;           /* DEVICE, LCUs + 1 records (tmvp_enable)                                             */
    uint32_t src_pitch_y, src_pitch_c;     /* samples                                                                            */
    int32_t ois_slot, me_slot;
    uint32_t tiles;
    uint32_t flags;                        /* SVT_AMD_MD_LAUNCH_*                                                                */
    uint32_t pad[2];                       /* 0                                                                                  */
} SvtAmdMdLaunchJob;                       /* 112 bytes */
typedef struct SvtAmdMdLaunchStatus {
    SvtAmdMdCtlCheck check;                /* of d_lcus                                                                          */
    uint32_t refused;                      /* 1: check.first_bad names an LCU - nothing of the picture was decided or encoded; 0 otherwise */
    uint32_t pad;                          /* written as 0                                                                       */
} SvtAmdMdLaunchStatus;                    /* 96 bytes */
#ifdef __cplusplus
static_assert(sizeof(SvtAmdMdLaunchJob) == 112 && sizeof(SvtAmdMdLaunchStatus) == 96, "launch records");
#else
_Static_assert(sizeof(SvtAmdMdLaunchJob) == 112 && sizeof(SvtAmdMdLaunchStatus) == 96, "launch records");
#endif
SVT_AMD_API int svt_amd_md_encode_picture_launch(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdLaunchJob *job, SvtAmdMdLaunchStatus *d_status);
/* The DEVICE arrays the last mode-decision call on `pic` - blocking or launched - wrote or is writing, one record per LCU in raster order: d_out SvtAmdMdLcuOut,
 * d_works SvtAmdLcuWork[16] at *work_stride bytes, d_results SvtAmdLcuResult[16] at *result_stride bytes; any of the five may be NULL.  They belong to the object
 * and live as long as it does; fetch what is wanted with svt_amd_device_download_async on the context the call ran on.  Refused on an object no mode-decision call
 * has touched. */
SVT_AMD_API int svt_amd_encdec_picture_md_records(SvtAmdEncDecPicture *pic, const SvtAmdMdLcuOut **d_out, const void **d_works, size_t *work_stride,
                                                  const void **d_results, size_t *result_stride);

/* ------------------------------------------------------------------------- */
/* Temporal motion field on the device: the co-located picture's field and intra-coded area from its work records */
/* ------------------------------------------------------------------------- */
/* The one closed-loop input of a P / B picture's mode decision: the motion field of its co-located picture (SvtAmdTmvpLcu above).  The field is nothing but the
 * final coding tree of that picture, and the device holds the tree: the SvtAmdLcuWork[16] records the mode-decision call (or svt_amd_encode_picture*) left in HBM.
 * What the reference does (tests/tmvp_numpy.py restates it; tests/golden/tmvp_*.npz hold its own results):
 *   EncodePass keeps the map for pictures with isUsedAsReferenceFlag (Codec/EbCodingLoop.c:3142-3158) and updates it per coded unit (:4500-4585): a unit at
 *   LCU-local (x, y) of size s writes the 16x16 map units vx in [(x + 15) >> 4, (x + s + 15) >> 4), vy likewise, at index vy * 4 + vx - a map unit takes the coded
 *   unit that contains its top-left sample; of four 8x8 units in a 16x16 only the top-left one writes, units at x or y = 8 (mod 16) write nothing.  An intra unit
 *   writes availabilityFlag = 0; an inter unit availabilityFlag = 1, predictionDirection = interPredDirectionIndex and, for each list the direction uses, mv[list]
 *   and refPicPOC[list] = the picture's own refPicPtrArray[list]->refPOC.  Everything else keeps what the pooled reference object held before.  The readers
 *   (GetTemporalMVP, GetTemporalMVP_V2, Codec/EbAdaptiveMotionVectorPrediction.c:1342-1386, :1412-1447) read only what the direction names, and never a unit whose
 *   top-left sample is outside the picture.
 *   intraCodedArea (Codec/EbCodingLoop.c:3264-3269, :3574; Codec/EbEncDecProcess.c:1887-1891): (EB_U8)((100 * sum of size^2 of the intra units) / (lumaWidth *
 *   lumaHeight)) in 32-bit unsigned arithmetic, 0 for an I picture.  (intraCodedAreaLCU has no reader and is not built.)
 * Here EVERY byte of the field is defined: the observable fields - `available`; `pred_dir` where available; mv[l] and ref_poc[l] of the lists the direction uses - as
 * above (a unit is inter when pred_mode == 1), everything else 0: units outside the picture, pred_dir / mv / ref_poc of unavailable units, the list a uni-predicted
 * unit does not use, and the whole record behind the last LCU (the mode-decision kernel reads record lcu and lcu + 1).
 * The intra-coded area serves two inputs that stay HOST bytes in this revision, SvtAmdMdInter.skip_cost_bias and SvtAmdMdcJob.ref_intra_coded_area: the host reads
 * the 8 bytes of SvtAmdRefStats per reference picture instead of walking its tree; reading them in place is a later step. */
typedef struct SvtAmdMotionFieldJob {
    const void *d_works;                   /* DEVICE: SvtAmdLcuWork or SvtAmdLcuWork16 of every LCU, raster order (heads and unit lists are shared); 4-byte aligned */
    size_t      work_stride;               /* sizeof the record type (any multiple of 4 that holds head and unit list, 1584 bytes: only those are read)            */
    uint16_t    width, height;             /* luma                                                                                                                   */
    uint8_t     slice_type;                /* EB_PICTURE of the picture the records belong to: 0 B, 1 P, 2 I                                                        */
    uint8_t     pad[3];                    /* 0                                                                                                                      */
    uint64_t    ref_poc[2];                /* its refPOC per list (unused lists: any value)                                                                          */
} SvtAmdMotionFieldJob;
typedef struct SvtAmdRefStats {
    uint32_t intra_area_sum;               /* sum of size^2 over the intra units (pred_mode == 2) of the picture                                                    */
    uint8_t  intra_coded_area;             /* EbReferenceObject_t.intraCodedArea: the percentage above, 0 for an I picture                                          */
    uint8_t  pad[3];                       /* written as 0                                                                                                           */
} SvtAmdRefStats;
#define SVT_AMD_MOTION_FIELD 0
#define SVT_AMD_MOTION_FIELD_STATS 1
/* bytes of the outputs: SVT_AMD_MOTION_FIELD (LCUs + 1) * sizeof(SvtAmdTmvpLcu), SVT_AMD_MOTION_FIELD_STATS sizeof(SvtAmdRefStats); 0 for anything else */
SVT_AMD_API size_t svt_amd_motion_field_bytes(uint16_t luma_width, uint16_t luma_height, int which);
/* Queues the field of one picture on the context's stream and returns: d_field (DEVICE, 8-byte aligned, svt_amd_motion_field_bytes) receives LCUs + 1 records,
 * nothing behind them is written; d_stats (DEVICE, or NULL) one SvtAmdRefStats.  Everything is checked before anything is queued (pictures of at most
 * SVT_AMD_MDCTL_MAX_LCUS LCUs - the picture may be of any size up to that, larger than the one the context was made for too: the entry reads no picture slot).
 * Per-LCU sums pass through a scratch the context owns (a word per LCU of the largest picture the entry takes, 64 KB, allocated at the first call): calls on
 * one context are stream-ordered among themselves, callers serialise per context as everywhere. */
SVT_AMD_API int svt_amd_motion_field_launch(SvtAmdContext *ctx, const SvtAmdMotionFieldJob *job, SvtAmdTmvpLcu *d_field, SvtAmdRefStats *d_stats);
/* The same from a picture object: the work records the LAST svt_amd_md_encode_picture[_inter][16] call on `pic` left on the device.  Refused when no such call has
 * completed on the object (or the last one was a P / B call without works and results: the mode decision alone, which writes no work records), and on an
 * object with a rank rectangle (svt_amd_encdec_picture_set_rect: the records of its other LCUs are zeroed, the field would be wrong).  ref_poc may be NULL for an I picture (slice_type 2).  Queued on ctx's stream: on the context the mode-decision call ran on, stream order suffices. */
SVT_AMD_API int svt_amd_encdec_picture_motion_field(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int slice_type, const uint64_t ref_poc[2], SvtAmdTmvpLcu *d_field,
                                                    SvtAmdRefStats *d_stats);
/* svt_amd_md_picture_set_controls for the motion field: binds a DEVICE array of LCUs + 1 records (svt_amd_motion_field_launch's output, or any array of that layout
 * whose last record is zero) as the co-located motion field of the NEXT svt_amd_md_encode_picture_inter[16] call on `pic`, and of that call only: every call on the
 * object consumes the binding, whether it succeeds or refuses.  That call passes tmvp == NULL; with X->tmvp_enable it points the kernel at the array - no upload, no
 * fill.  One that passes a host tmvp as well is refused and drops the binding; with tmvp_enable == 0 or X == NULL the binding is dropped unread; d_field == NULL drops a
 * binding.  Without a binding, tmvp == NULL with tmvp_enable is refused as before.  Ordering as for svt_amd_md_picture_set_controls: written on the context the call
 * runs on, stream order suffices; across lanes it is the caller's.  The array must stay valid until the blocking call returns.  May be combined with a controls
 * binding in the same call. */
SVT_AMD_API int svt_amd_md_picture_set_motion_field(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdTmvpLcu *d_field);
/* debug: stage clocks of the mode-decision kernel (16 shader-clock sums per LCU, accumulated over the picture object's later calls; the first call
 * switches the collection on) - see svt-hevc_amd/csrc/md_kernels.hip */
SVT_AMD_API int svt_amd_debug_md_profile(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out);
SVT_AMD_API int svt_amd_debug_md_profile_sub(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out);
/* ... and both sets of sums by the depth of the coding unit they were spent on: out[LCU][depth 0..3][32] */
SVT_AMD_API int svt_amd_debug_md_profile_depth(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out);
/* debug / test: the full loops' 16x16 and 32x32 forward transforms on the register butterflies (on != 0) instead of the matrix cores for the picture object's later calls:
 * both paths must give the reference's decisions (tests/test_gpu_md.py) */
SVT_AMD_API int svt_amd_debug_md_force_butterflies(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int on);
/* development builds (-DMD_TRACE) only, SVT_AMD_ERR_BAD_PARAM otherwise: lane-0 time stamps of the kernel's four waves along two units of one LCU (tools/md_trace.py) */
SVT_AMD_API int svt_amd_debug_md_trace(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int lcu, int unit, unsigned long long *out);
/* measurement: duration in ms (HIP events on the call's stream) and launch width (workgroups) of the picture object's last mode-decision kernel launch */
SVT_AMD_API int svt_amd_debug_md_kernel_ms(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, float *ms, int *workgroups);
/* ... and of the encode-pass kernel queued behind it by the same call */
SVT_AMD_API int svt_amd_debug_md_ep_ms(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, float *ms);
/* diagnosis: the mode-decision launches that hold (or wait for) workgroups of the device budget right now (md_picture.hip: MdFlight) */
SVT_AMD_API int svt_amd_debug_md_flights(int *in_flight, int *workgroups_held, int *waiting);
/* Everything the first svt_amd_md_encode_picture[_inter / 16] call on a picture object would allocate (device state, page-locked staging, events), made NOW: for hosts that
 * build their picture objects before their clock starts (the encoder binding at EbInitEncoder time) - allocations made while other pictures' kernels run wait for them. */
SVT_AMD_API int svt_amd_md_picture_warmup(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic);
/* measurement: dynamic LDS bytes a workgroup of k_md_picture<inter, sample bytes> is launched with (the whole LCU state: one workgroup per CU) */
SVT_AMD_API int svt_amd_debug_md_kernel_lds_bytes(int inter, int bytes_per_sample);
/* test: the motion-vector candidate lists of the P / B unit loop (md_kernels.hip: the register form of GenerateL0L1AmvpMergeLists + ChooseMVPIdx_V2) on single
 * units, a lane per job - the __device__ functions the unit loop calls, on inputs no recorded picture holds (tests/test_gpu_md_lists.py against the reference's
 * own outputs, tests/golden/mvlists_seeded.npz).  Nothing of the product calls it. */
typedef struct SvtAmdMdListNb {            /* a spatial neighbour: MvUnit_t + whether the derivation may use it (the caller derives that)                     */
    int16_t mv[2][2];                      /* [list]{x, y}                                                                                                    */
    uint8_t dir, avail, pad[2];            /* 0 list 0, 1 list 1, 2 both                                                                                      */
} SvtAmdMdListNb;
typedef struct SvtAmdMdListJob {
    uint16_t width, height;                /* the picture, luma                                                                                               */
    uint16_t ox, oy;                       /* the unit's origin in the picture (a multiple of size)                                                           */
    uint8_t size;                          /* 8, 16, 32, 64                                                                                                   */
    uint8_t slice_type;                    /* 0 B, 1 P                                                                                                        */
    uint8_t colocated_pu_ref_list, is_low_delay;
    uint8_t has_field;                     /* a co-located motion field exists (SvtAmdMdInter.tmvp_enable)                                                    */
    uint8_t total_merge;                   /* the merge candidates wanted: 2, 3 or 5 (md_nmm)                                                                 */
    uint8_t tile_left, tile_top, tile_right; /* the LCU's tile-edge flags: what `avail` was derived with; the device and the CPU checker do not read them    */
    uint8_t me_dir;                        /* the motion-estimation candidate: direction ...                                                                  */
    uint16_t pool[2];                      /* the co-located field of this LCU and of the LCU to its right: indices into the pool of SvtAmdTmvpLcu records    */
    int16_t me_mv[2][2];                   /* ... and vectors [list]{x, y}                                                                                    */
    uint8_t pad[2];
    uint64_t picture_number, ref_poc[2], colocated_poc;
    SvtAmdMdListNb nb[5];                  /* A0, A1, B0, B1, B2                                                                                              */
    uint8_t pad2[4];
} SvtAmdMdListJob;
typedef struct SvtAmdMdListOut {
    int16_t amvp[2][2][2];                 /* [list][index]{x, y}: entries below amvp_count[list] are meaningful                                             */
    uint8_t amvp_count[2];
    uint8_t merge_count;
    uint8_t mvp_idx[2];                    /* of the lists me_dir uses                                                                                        */
    uint8_t merge_dir[5];
    int16_t merge_mv[5][2][2];             /* [candidate][list]{x, y}: the lists merge_dir uses are meaningful                                                */
    int16_t cand_mv[2][2];                 /* me_mv after ClipMV, of the lists me_dir uses                                                                    */
    int16_t mvp[2][2];                     /* the chosen predictors                                                                                           */
    uint8_t pad[14];
} SvtAmdMdListOut;
#ifdef __cplusplus
static_assert(sizeof(SvtAmdMdListNb) == 12 && sizeof(SvtAmdMdListJob) == 128 && sizeof(SvtAmdMdListOut) == 96, "tests mirror these layouts as numpy dtypes");
#else
_Static_assert(sizeof(SvtAmdMdListNb) == 12 && sizeof(SvtAmdMdListJob) == 128 && sizeof(SvtAmdMdListOut) == 96, "tests mirror these layouts as numpy dtypes");
#endif
/* d_jobs, d_pool, d_outs: DEVICE arrays (n jobs, the pool the jobs index, n outs).  One launch on the context's stream; the caller synchronises.  A NULL pointer or
 * n == 0: SVT_AMD_ERR_BAD_PARAM, nothing queued.  Every byte of outs [0, n) is written, nothing behind them.  The jobs live on the device, so their pool indices are
 * NOT checked: both of every job must lie inside d_pool (also where has_field is 0). */
SVT_AMD_API int svt_amd_debug_md_lists_batch(SvtAmdContext *ctx, const SvtAmdMdListJob *d_jobs, const SvtAmdTmvpLcu *d_pool, SvtAmdMdListOut *d_outs, uint32_t n);
/* measurement: LDS bytes (static + dynamic) a workgroup of the motion-estimation kernel of `phase` (0 = HME, 1 = search) is launched with for a job with
 * these controls; params == NULL: what the last svt_amd_me_* launch of the process requested (compiler's static size + the launcher's pool) */
SVT_AMD_API int svt_amd_debug_me_kernel_lds_bytes(const SvtAmdMeParams *params, int phase);
/* measurement: what the context's device makes of that kernel at 256 threads and that job's pool: resident workgroups per CU
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor) and the kernel's private segment in bytes per lane (localSizeBytes of hipFuncGetAttributes: 0 = no scratch frame) */
SVT_AMD_API int svt_amd_debug_me_kernel_occupancy(SvtAmdContext *ctx, const SvtAmdMeParams *params, int phase, int *workgroups_per_cu, int *private_bytes);
/* measurement: the completion markers this context (lane) has recorded behind its ME / OIS launches since it was made - one per launch, however many pictures the
 * launch holds; the marker behind a kernel that READ a slot's records in place is not counted - and every wait on another lane's marker it has issued: as a consumer
 * of records left in the slots (me == NULL / ois == NULL, an OIS launch reading the slot's ME records), as the next marker of a chain (a band of a picture whose
 * other bands another lane wrote, a second reader of one slot), and as a launch into a slot whose records another lane is still reading */
SVT_AMD_API int svt_amd_debug_launch_markers(SvtAmdContext *ctx, unsigned long long *records, unsigned long long *waits);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HEVC_AMD_H */
