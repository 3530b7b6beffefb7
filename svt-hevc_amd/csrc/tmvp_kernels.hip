/*
 * tmvp_kernels.hip - the temporal motion field of a coded picture (SvtAmdTmvpLcu, 416 bytes an LCU) and its intra-coded area, built on the device from the
 * final coding trees the mode-decision / encode-pass calls leave in HBM (SvtAmdLcuWork[16]), in the stream-ordered shape of mdctl_kernels.hip / irc_kernels.hip
 * (include/svt_hevc_amd.h "Temporal motion field on the device"): what EncodePass writes into the reference object's tmvpMap unit by unit
 * (Codec/EbCodingLoop.c:3142-3158, :4500-4585) as its readers see it (GetTemporalMVP / GetTemporalMVP_V2, Codec/EbAdaptiveMotionVectorPrediction.c:1342-1386,
 * :1412-1447), and the intraCodedArea of CopyStatisticsToRefObject (Codec/EbCodingLoop.c:3264-3269, :3574; Codec/EbEncDecProcess.c:1887-1891).  Integer logic on
 * the 48-byte head and the unit list of a record; no sample is read.  Restated as tests/tmvp_numpy.py spells it out.
 *   k_tmvp_lcu    grid ((LCUs + 1) / 4 rounded up), a wave per record of the field.  Lane k holds unit k of the LCU's list (six words); lane u < 16 speaks for the
 *                 16x16 map unit u and finds the coded unit that contains its top-left sample (a walk over the list, unit k's geometry broadcast from
 *                 lane k) - the reference's write range [(x + 15) >> 4, (x + s + 15) >> 4) says the same: of four 8x8 units only the top-left one, none at
 *                 x or y = 8 mod 16.  The 416-byte record is built in LDS (zeroed first: units
 *                 outside the picture, intra units, the unused list of a uni-predicted unit and the record behind the last LCU stay 0) and leaves as 104
 *                 coalesced words.  The LCU's sum of intra unit areas goes into the context's scratch, a word per LCU.
 *   k_tmvp_stats  grid (1), a workgroup of 256 threads: totals the per-LCU sums and writes SvtAmdRefStats in the reference's 32-bit arithmetic.
 * No atomics, nothing to zero.  Bound: latency - 416 bytes written and at most 1584 read per LCU.
 */
#include "pa_batch.h"

#define TMVP_HEAD_BYTES offsetof(SvtAmdLcuWork, cu)   /* 48 */
#define TMVP_LIST_BYTES offsetof(SvtAmdLcuWork, src_y) /* head + unit list: all a record is read of */
#define TMVP_WORDS (sizeof(SvtAmdTmvpLcu) / 4)
#define TMVP_STATS_THREADS 256
static_assert(sizeof(SvtAmdTmvpLcu) == 416 && offsetof(SvtAmdTmvpLcu, ref_poc) == 128 && offsetof(SvtAmdTmvpLcu, pred_dir) == 384 && offsetof(SvtAmdTmvpLcu, available) == 400,
              "SvtAmdTmvpLcu layout");
static_assert(sizeof(SvtAmdLcuCu) == 24 && offsetof(SvtAmdLcuCu, pred_mode) == 3 && offsetof(SvtAmdLcuCu, inter_dir) == 10 && offsetof(SvtAmdLcuCu, mv) == 16, "SvtAmdLcuCu layout");
static_assert(TMVP_HEAD_BYTES == 48 && TMVP_LIST_BYTES == 1584 && offsetof(SvtAmdLcuWork, num_cus) == 4 && offsetof(SvtAmdLcuWork16, cu) == TMVP_HEAD_BYTES &&
              offsetof(SvtAmdLcuWork16, src_y) == TMVP_LIST_BYTES, "the 8- and 16-bit work records share head and unit list");
static_assert(sizeof(SvtAmdMotionFieldJob) == 40 && sizeof(SvtAmdRefStats) == 8, "motion-field records");

/* grid ((lcus + 1 + 3) / 4): one wave per record, record `lcus` is the zero record the mode decision reads behind the last LCU */
__global__ __launch_bounds__(256) void k_tmvp_lcu(const uint8_t *__restrict__ works, size_t stride, int width, int height, int lcus_w, int lcus, unsigned long long poc0,
                                                  unsigned long long poc1, uint32_t *__restrict__ field, uint32_t *__restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_rec[4][TMVP_WORDS];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int r = (int)blockIdx.x * 4 + wave;
    const bool active = r <= lcus, coded = r < lcus; /* wave-uniform */
    const int n = coded ? r : lcus - 1;              /* a wave at or past the zero record reads the last LCU and keeps nothing of it */
    const int ox = (n % lcus_w) * 64, oy = (n / lcus_w) * 64;
    uint32_t *rec = s_rec[wave];
    uint8_t *rec8 = (uint8_t *)rec;

    rec[b] = 0u;
    if (b + 64 < (int)TMVP_WORDS)
        rec[b + 64] = 0u;

    /* lane k: unit k of the list */
    const uint8_t *work = works + (size_t)n * stride;
    int count = __builtin_amdgcn_readfirstlane((int)work[offsetof(SvtAmdLcuWork, num_cus)]); /* one value a wave: the walk below is a scalar loop */
    count = count > SVT_AMD_LCU_MAX_CUS ? SVT_AMD_LCU_MAX_CUS : count;
    uint32_t geo = 0, dir = 0, mv0 = 0, mv1 = 0;
    if (b < count) {
        const uint32_t *cu = (const uint32_t *)(work + TMVP_HEAD_BYTES + (size_t)b * sizeof(SvtAmdLcuCu));
        geo = cu[0], dir = cu[2] >> 16 & 0xFFu, mv0 = cu[4], mv1 = cu[5];
    }
    const int size = (int)(geo >> 16 & 0xFFu), mode = (int)(geo >> 24);
    /* the LCU's intra area: size^2 of its intra units */
    uint32_t area = b < count && mode == 2 ? (uint32_t)(size * size) : 0u;
    for (int o = 32; o > 0; o >>= 1)
        area += (uint32_t)__shfl_xor((int)area, o);
    if (coded && b == 0)
        sums[n] = area;

    /* lane u < 16: the coded unit that contains the top-left sample of map unit u, the first of the list if the list is no partition.  The walk broadcasts unit k's
     * geometry from lane k (k is wave-uniform); the lanes from 16 on speak for no map unit - their `found` is never kept - but stay in the walk and in the four
     * fetches below, whose source lanes (any unit of the list) must be active */
    const int px = (b & 3) * 16, py = (b >> 2 & 3) * 16;
    int found = -1;
    for (int k = 0; k < count; k++) {
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)geo, k);
        const int x = (int)(g & 0xFFu), y = (int)(g >> 8 & 0xFFu), s = (int)(g >> 16 & 0xFFu);
        if (found < 0 && px >= x && px < x + s && py >= y && py < y + s)
            found = k;
    }
    const int at = found < 0 ? 0 : found;
    const uint32_t f_geo = (uint32_t)__shfl((int)geo, at), f_dir = (uint32_t)__shfl((int)dir, at);
    const uint32_t f_mv[2] = {(uint32_t)__shfl((int)mv0, at), (uint32_t)__shfl((int)mv1, at)};
    __syncthreads();
    if (coded && b < 16 && found >= 0 && ox + px < width && oy + py < height && f_geo >> 24 == 1u) { /* an inter unit; everything else stays unavailable and 0 */
        rec8[offsetof(SvtAmdTmvpLcu, available) + b] = 1;
        rec8[offsetof(SvtAmdTmvpLcu, pred_dir) + b] = (uint8_t)f_dir;
        const unsigned long long poc[2] = {poc0, poc1};
#pragma unroll
        for (int l = 0; l < 2; l++)
            if (f_dir == 2u || f_dir == (uint32_t)l) { /* UNI_PRED_LIST_0 0, UNI_PRED_LIST_1 1, BI_PRED 2 */
                rec[l * 16 + b] = f_mv[l];
                rec[32 + 2 * (l * 16 + b)] = (uint32_t)poc[l], rec[32 + 2 * (l * 16 + b) + 1] = (uint32_t)(poc[l] >> 32);
            }
    }
    __syncthreads();
    if (active) {
        uint32_t *dst = field + (size_t)r * TMVP_WORDS;
        dst[b] = rec[b];
        if (b + 64 < (int)TMVP_WORDS)
            dst[b + 64] = rec[b + 64];
    }
}

/* grid (1): (EB_U8)((100 * sum) / (width * height)) in 32-bit unsigned arithmetic, 0 for an I picture */
__global__ __launch_bounds__(TMVP_STATS_THREADS) void k_tmvp_stats(const uint32_t *__restrict__ sums, int lcus, uint32_t luma_samples, int slice_type, SvtAmdRefStats *__restrict__ out)
{
    __shared__ uint32_t s_part[TMVP_STATS_THREADS / 64];
    const int t = threadIdx.x;
    uint32_t acc = 0;
    for (int i = t; i < lcus; i += TMVP_STATS_THREADS)
        acc += sums[i];
    for (int o = 32; o > 0; o >>= 1)
        acc += (uint32_t)__shfl_xor((int)acc, o);
    if ((t & 63) == 0)
        s_part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < TMVP_STATS_THREADS / 64; w++)
            sum += s_part[w];
        SvtAmdRefStats s;
        s.intra_area_sum = sum;
        s.intra_coded_area = slice_type == 2 ? 0 : (uint8_t)((100u * sum) / luma_samples);
        s.pad[0] = s.pad[1] = s.pad[2] = 0;
        *out = s;
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

extern "C" size_t svt_amd_motion_field_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    if (luma_width < 1 || luma_height < 1)
        return 0;
    return which == SVT_AMD_MOTION_FIELD ? ((size_t)svt_amd_lcu_count(luma_width, luma_height) + 1) * sizeof(SvtAmdTmvpLcu) : which == SVT_AMD_MOTION_FIELD_STATS ?
           sizeof(SvtAmdRefStats) : 0;
}

extern "C" int svt_amd_motion_field_launch(SvtAmdContext *ctx, const SvtAmdMotionFieldJob *job, SvtAmdTmvpLcu *d_field, SvtAmdRefStats *d_stats)
{
    /* ---- everything is checked before anything is queued ---- */
    if (!ctx || !job || !d_field)
        SVT_AMD_BAD("%s: a context, a job and a device array for the field", __func__);
    const int w = job->width, h = job->height, wl = (w + 63) / 64, hl = (h + 63) / 64, lcus = wl * hl;
    if (!job->d_works)
        SVT_AMD_BAD("%s: the job has no work records", __func__);
    if (job->work_stride < TMVP_LIST_BYTES || job->work_stride % 4 || (uintptr_t)job->d_works % 4)
        SVT_AMD_BAD("%s: work records %zu bytes apart at %p (at least the %zu bytes of head and unit list, words)", __func__, job->work_stride, job->d_works,
                    (size_t)TMVP_LIST_BYTES);
    if (w < 1 || h < 1 || lcus > SVT_AMD_MDCTL_MAX_LCUS)
        SVT_AMD_BAD("%s: a picture of %dx%d (at most %d LCUs)", __func__, w, h, SVT_AMD_MDCTL_MAX_LCUS);
    if (job->slice_type > 2)
        SVT_AMD_BAD("%s: slice type %d", __func__, job->slice_type);
    if (job->pad[0] || job->pad[1] || job->pad[2])
        SVT_AMD_BAD("%s: a pad byte is not 0", __func__);
    if ((uintptr_t)d_field % 8 || (uintptr_t)d_stats % 4)
        SVT_AMD_BAD("%s: the field at %p (8-byte aligned: ref_poc) or the statistics at %p (4-byte aligned)", __func__, (void *)d_field, (void *)d_stats);

    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->d_tmvp) /* the per-LCU intra sums: a word per LCU of the largest picture the entry takes */
        HIP_TRY(hipMalloc(&ctx->d_tmvp, sizeof(uint32_t) * SVT_AMD_MDCTL_MAX_LCUS));
    hipStream_t st = svt_amd_ctx_stream(ctx);
    uint32_t *d_sums = (uint32_t *)ctx->d_tmvp;
    hipLaunchKernelGGL(k_tmvp_lcu, dim3((unsigned)(lcus + 1 + 3) / 4), dim3(256), 0, st, (const uint8_t *)job->d_works, job->work_stride, w, h, wl, lcus,
                       (unsigned long long)job->ref_poc[0], (unsigned long long)job->ref_poc[1], (uint32_t *)d_field, d_sums);
    HIP_TRY(hipGetLastError());
    if (d_stats) {
        hipLaunchKernelGGL(k_tmvp_stats, dim3(1), dim3(TMVP_STATS_THREADS), 0, st, (const uint32_t *)d_sums, lcus, (uint32_t)w * (uint32_t)h, (int)job->slice_type, d_stats);
        HIP_TRY(hipGetLastError());
    }
    return SVT_AMD_OK;
}
