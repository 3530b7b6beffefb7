/* md_picture.h - where the two translation units of the device-resident mode decision meet (not part of the C-ABI): md_kernels.hip (with the five headers of its device code, md_state.h .. md_units_inter.h) holds every kernel and __device__
 * function, md_picture.hip the picture state, the launch budget and the entries.  The picture's descriptor as the kernel reads it, and what the kernel unit offers the
 * host unit; nothing else crosses. */
#ifndef SVT_AMD_MD_PICTURE_H
#define SVT_AMD_MD_PICTURE_H
#include "encdec_device.h"
struct MdPictureDev {
    uint8_t *md_rec;              /* the mode decision's luma reconstruction, sample (0,0) */
    uint32_t md_pitch;
    uint32_t *md_info;            /* per 4x4 luma block: mode type | intra luma mode << 8 | depth << 16 | skip flag << 24; ~0 = never written */
    uint32_t info_pitch;
    const uint8_t *src[3];        /* source planes on the device, sample (0,0) */
    uint32_t src_pitch[2];
    const SvtAmdOisLcuResult *ois;
    const SvtAmdMdLcu *lcus;
    const SvtAmdMdPicture *P;
    SvtAmdMdLcuOut *out;
    /* P / B pictures */
    uint4 *md_mv;                 /* per 8x8 luma block: the unit's MvUnit_t {mv[0], mv[1], direction} (mdMvNeighborArray) */
    uint32_t mv_pitch;
    const SvtAmdMdInter *X;
    const SvtAmdMeLcuResult *me;
    const SvtAmdTmvpLcu *tmvp;
    int encode;                   /* 0: mode decision only (no work record, no encode pass) */
    const SvtAmdCabacCost *cost;  /* the picture's coefficient-rate tables (the picture object's d_cost) */
    /* The mode decision works on 8-bit samples whatever the encoder's bit depth (Inter2Nx2NPuPredictionHevc narrows the 16-bit reference block it reads,
     * UnPackReferenceBlock, Codec/EbInterPrediction.c:414-457; the source is the picture's 8-bit plane): mref = the reference pictures as the mode decision reads them -
     * the picture object's own of an 8-bit picture, their 8-MSB views of a 10-bit one -, src16 = the 10-bit source the encode pass behind it codes (null: 8-bit). */
    EpRefPlanes mref[2];
    const uint16_t *src16[3];
    unsigned long long *prof;     /* debug (svt_amd_debug_md_profile): 16 shader-clock sums per LCU, or null */
    int prof_lcus;                /* LCUs of the picture: the sub-stage sums start behind the stage sums of all of them */
    int force_butterflies;        /* debug (svt_amd_debug_md_force_butterflies): the 16x16 / 32x32 forward transforms of the full loops on the register butterflies (the path a unit
                                   * outside the matrix-core form's wrap-free domain takes) - the tests run the fixtures both ways */
    unsigned long long *trace;    /* debug (-DMD_TRACE builds, svt_amd_debug_md_trace): the time stamps of trace_lcu's units [trace_unit, trace_unit + 2), or null */
    int trace_lcu, trace_unit;
};

/* ---- what md_kernels.hip offers md_picture.hip ---- */

/* The estimator's scan / context tables into the constant memory k_md_picture reads (rate_device.h: c_rt and rate_tables_once are static, a copy per translation unit -
 * this is the kernel unit's).  The first call per device is a synchronising copy: the entries and svt_amd_md_picture_warmup call it, the launch below does not */
int svt_amd_md_kernel_rate_tables(int device);

/* one launch of k_md_picture: `grid` workgroups over the n_active LCUs of `order` */
struct MdPictureLaunch {
    hipStream_t st;
    int grid;
    const MdPictureDev *d_D;
    void *d_works;                /* SvtAmdLcuWork / SvtAmdLcuWork16 records by bps */
    int n_active, wl;
    unsigned *ticket, *md_done;
    const unsigned *order;
    unsigned epoch;
    bool inter, ifree, profiled;  /* which instance: P / B, coded without sub-sample search, with the stage marks */
    uint32_t bps;
};
int svt_amd_md_kernel_launch(const MdPictureLaunch &l);

/* The two plane kernels (they are scheduled like the unit they have always been compiled in).  k_msb_view: the 8-MSB view of `samples` 16-bit samples;
 * k_md_fetch_plane: `bytes` bytes of a plane in page-locked host memory, as the device sees it, into HBM by `workgroups` workgroups */
int svt_amd_md_kernel_msb_view(hipStream_t st, const void *in16, uint8_t *out8, size_t samples);
int svt_amd_md_kernel_fetch_plane(hipStream_t st, int workgroups, uint8_t *d_dst, const uint8_t *src, size_t bytes);

/* k_md_lists_batch (svt_amd_debug_md_lists_batch): a lane per job */
int svt_amd_md_kernel_lists_batch(hipStream_t st, const SvtAmdMdListJob *d_jobs, const SvtAmdTmvpLcu *d_pool, SvtAmdMdListOut *d_outs, uint32_t n);

/* svt_amd_debug_md_kernel_lds_bytes: the LCU state of the I (inter == 0) or P / B kernel and the descriptor beside it */
int svt_amd_md_kernel_lds_bytes(int inter);

/* svt_amd_debug_md_trace: the 64-bit words a -DMD_TRACE build of the kernel unit writes per traced LCU; 0 in every other build */
int svt_amd_md_kernel_trace_words(void);

#endif
