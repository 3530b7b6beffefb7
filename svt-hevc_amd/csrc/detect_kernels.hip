/*
 * detect_kernels.hip - the second half of GatheringPictureStatistics (Codec/EbPictureAnalysisProcess.c:3995) in the batched, stream-ordered shape of
 * side_kernels.hip (include/svt_hevc_amd.h "Batched chroma statistics" / "Batched picture detectors"): the picture is a grid dimension, the per-picture
 * pointers come from a descriptor table in device memory, nothing is copied to the host.
 *   k_chroma_means        ComputeChromaBlockMean (:1448) / ZeroOutChromaBlockMean (:1383): grid (LCUs, pictures), one wave per LCU, 32 lanes: lane = (plane,
 *                         8x8 chroma block); four 8-byte loads (rows 0, 2, 4, 6: ComputeSubMean8x8_SSE2_INTRIN) + v_sad_u8 against zero, the 32x32 / 64x64
 *                         levels by lane shuffles.  No LDS, no scratch.
 *   k_chroma_hist(_finish) SubSampleChromaGeneratePixelIntensityHistogramBins (:3440): grid (strips, regions, pictures), both planes per workgroup; LDS bins
 *                         merged into the output with vector atomics; the finish kernel applies the start value, the shift and the averages.
 *   k_detect_lcu          DetermineHomogeneousRegionInPicture (:3751) and the per-LCU half of EdgeDetection (:3627): grid (LCUs, pictures), one wave per LCU, a
 *                         lane per 8x8 variance; 64-bit sums by lane shuffles; the picture's variance sum, low-variance count and maxGrad
 *                         (EdgeDetectionMeanLumaChroma16x16, :3522) by vector atomics into the context's scratch.
 *   k_detect_edge         what needs the reduced values but no other LCU: edge_block_num (70 % of picAvgVariance) and the 16x16 edge map against maxGrad; grid
 *                         (LCUs / 4, pictures), a wave per LCU, a lane per 16x16 unit; the edge LCUs are counted by a vector atomic.
 *   k_detect_finish       what needs other LCUs or the counts: grid (pictures), a workgroup per picture; the LCUs' 64x64 means and trigger flags in LDS for the
 *                         9x9 gather of isolatedHighIntensityLcu, then the picture record.
 * Bound: HBM / latency - 1/4 B/pel (means, the even rows of both planes: half of the 1/2 B/pel chroma), 1/32 B/pel touched lines for the histograms, 256 B per LCU
 * for the detectors.
 */
#include "pa_batch.h"
#include <string.h>

struct ChromaJobDev {
    const uint8_t *cb, *cr;        /* null: nothing of this picture */
    SvtAmdPaLcuChroma *means;      /* [lcus] or null */
    uint32_t *hist;                /* [regions][2][256] or null */
    unsigned long long *sums;      /* [regions][2]: context-owned scratch, zeroed by the call */
    uint8_t *region_avg;           /* [64][2] or null */
    unsigned long long *total;     /* [2] or null */
    int32_t pitch;
    int32_t pad;
};
static_assert(sizeof(ChromaJobDev) == 64, "ChromaJobDev layout");
#define CHROMA_SUMS_BYTES ((size_t)SVT_AMD_MAX_BATCH * 64 * 2 * 8)
#define CHROMA_STRIPS 8

struct DetectReduce {
    unsigned long long var_sum;    /* picTotVariance (:3930) */
    uint32_t low_var;              /* veryLowVarCnt (:3784) */
    uint32_t max_grad;             /* maxGrad (:3595); 0 = nothing above the start value 1 */
    uint32_t edge_lcus;            /* numberOfEdgeLcu (:3738): k_detect_edge counts, k_detect_finish reads */
    uint32_t pad[3];
};
static_assert(sizeof(DetectReduce) == 32, "DetectReduce layout");
struct DetectJobDev {
    const SvtAmdPaLcuStats *stats;
    const SvtAmdPaLcuChroma *chroma; /* null: no 16x16 edge map for this picture */
    SvtAmdPaLcuDetect *lcu;
    SvtAmdPaPicDetect *pic;
    DetectReduce *red;             /* context-owned scratch, zeroed by the call */
    int32_t logo_cols, logo_rows;  /* the potentialLogoLcu map of the resolution class, in LCUs (Codec/EbSequenceControlSet.c:253-272) */
};
static_assert(sizeof(DetectJobDev) == 48, "DetectJobDev layout");
#define DETECT_RED_BYTES (sizeof(DetectReduce) * SVT_AMD_MAX_BATCH)
#define DETECT_MAX_LCUS 16384

struct __attribute__((packed, aligned(1))) Row8 { /* an 8-byte row at any address: chroma planes are unpadded, their pitch is the caller's */
    uint32_t x, y;
};

/* ---------------------------------------------------------------- chroma block means ---------------------------------------------------------------- */

__global__ __launch_bounds__(32) void k_chroma_means(const ChromaJobDev *__restrict__ jobs, int width, int height, int lcus_w)
{
    const ChromaJobDev &J = jobs[blockIdx.y];
    if (!J.means)
        return;
    const int lcu = blockIdx.x, t = threadIdx.x, lx = (lcu % lcus_w) * 64, ly = (lcu / lcus_w) * 64;
    uint32_t *o32 = (uint32_t *)&J.means[lcu];
    if (lx + 64 > width || ly + 64 > height) { /* ZeroOutChromaBlockMean; the padding bytes with it */
        if (t < 12)
            o32[t] = 0u;
        return;
    }
    const int plane = t >> 4, k = t & 15; /* k: the 16x16 luma unit = 8x8 chroma block, raster */
    const uint8_t *p = (plane ? J.cr : J.cb) + (size_t)((ly >> 1) + (k >> 2) * 8) * J.pitch + (lx >> 1) + (k & 3) * 8;
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < 8; r += 2) {
        const Row8 row = *(const Row8 *)(p + (size_t)r * J.pitch);
        sum = __builtin_amdgcn_sad_u8(row.x, 0u, sum);
        sum = __builtin_amdgcn_sad_u8(row.y, 0u, sum);
    }
    const uint32_t m16 = sum << 3; /* 8 fractional bits */
    /* 32x32: the four 16x16 of it differ in bits 0 and 2 of k */
    uint32_t m32 = m16 + __shfl_xor(m16, 1);
    m32 = (m32 + __shfl_xor(m32, 4)) >> 2;
    /* 64x64 as the reference has it: blocks 0, 1, 3 and 3 again (:1586-1587) - block 2 is never read */
    const int base = plane << 4;
    const uint32_t q0 = __shfl(m32, base), q1 = __shfl(m32, base + 2), q3 = __shfl(m32, base + 10);
    const uint32_t m64 = (q0 + q1 + q3 + q3) >> 2;
    uint8_t *o = plane ? J.means[lcu].cr_mean : J.means[lcu].cb_mean;
    o[5 + k] = (uint8_t)(m16 >> 8);
    if (!(k & 5))
        o[1 + ((k >> 3) << 1) + ((k >> 1) & 1)] = (uint8_t)(m32 >> 8);
    if (k == 0)
        o[0] = (uint8_t)(m64 >> 8);
    if (t < 6)
        J.means[lcu].pad[t] = 0;
}

/* ---------------------------------------------------------------- chroma region histograms ---------------------------------------------------------------- */

/* the luma region (a, b) -> its chroma origin and the number of counted columns / rows (every 4th of the area, the area = the luma region size >> 1) */
__device__ __forceinline__ void chroma_region(int width, int height, int regions_w, int regions_h, int a, int b, int *cx, int *cy, int *cols, int *rows,
                                              unsigned long long *luma_area)
{
    const int rw = width / regions_w, rh = height / regions_h;
    const int w = a == regions_w - 1 ? width - a * rw : rw, h = b == regions_h - 1 ? height - b * rh : rh;
    *cx = (a * rw) >> 1, *cy = (b * rh) >> 1;
    *cols = ((w >> 1) + 3) >> 2, *rows = ((h >> 1) + 3) >> 2;
    *luma_area = (unsigned long long)w * (unsigned long long)h;
}

/* grid (strips, regions, pictures); width / height: luma */
__global__ __launch_bounds__(256) void k_chroma_hist(const ChromaJobDev *__restrict__ jobs, int width, int height, int regions_w, int regions_h)
{
    const ChromaJobDev &J = jobs[blockIdx.z];
    if (!J.hist)
        return;
    __shared__ uint32_t bins[2][256];
    __shared__ unsigned long long s_sum[2];
    const int t = threadIdx.x, region = blockIdx.y, a = region / regions_h, b = region - a * regions_h;
    int cx, cy, cols, rows;
    unsigned long long area;
    chroma_region(width, height, regions_w, regions_h, a, b, &cx, &cy, &cols, &rows, &area);
    bins[0][t] = bins[1][t] = 0;
    if (t < 2)
        s_sum[t] = 0;
    __syncthreads();
    const int strips = gridDim.x, per = (rows + strips - 1) / strips;
    const int rs = (int)blockIdx.x * per, re = min(rs + per, rows);
    const int pitch = J.pitch;
    unsigned long long sum_b = 0, sum_r = 0;
    for (int i = t; i < (re > rs ? (re - rs) * cols : 0); i += 256) {
        const size_t at = (size_t)(cy + 4 * (rs + i / cols)) * pitch + cx + 4 * (i % cols);
        const uint32_t vb = J.cb[at], vr = J.cr[at];
        atomicAdd(&bins[0][vb], 1u);
        atomicAdd(&bins[1][vr], 1u);
        sum_b += vb, sum_r += vr;
    }
    for (int o = 32; o > 0; o >>= 1)
        sum_b += __shfl_xor(sum_b, o), sum_r += __shfl_xor(sum_r, o);
    if ((t & 63) == 0) {
        if (sum_b)
            atomicAdd(&s_sum[0], sum_b);
        if (sum_r)
            atomicAdd(&s_sum[1], sum_r);
    }
    __syncthreads();
    for (int c = 0; c < 2; c++)
        if (bins[c][t])
            atomicAdd(&J.hist[(region * 2 + c) * 256 + t], bins[c][t]);
    if (t < 2 && s_sum[t])
        atomicAdd(&J.sums[region * 2 + t], s_sum[t]);
}

/* grid (regions, pictures) */
__global__ __launch_bounds__(256) void k_chroma_hist_finish(const ChromaJobDev *__restrict__ jobs, int width, int height, int regions_w, int regions_h)
{
    const ChromaJobDev &J = jobs[blockIdx.y];
    if (!J.hist)
        return;
    const int region = blockIdx.x, t = threadIdx.x, a = region / regions_h, b = region - a * regions_h;
    for (int c = 0; c < 2; c++) /* bins start at 1 (InitializeBuffer_32bits ... 1) and end << decimStep (:3493) */
        J.hist[(region * 2 + c) * 256 + t] = (J.hist[(region * 2 + c) * 256 + t] + 1u) << 4;
    if (t < 2) {
        int cx, cy, cols, rows;
        unsigned long long area;
        chroma_region(width, height, regions_w, regions_h, a, b, &cx, &cy, &cols, &rows, &area);
        const unsigned long long sum = J.sums[region * 2 + t] << 4; /* sum << decimStep (:3489) */
        if (J.region_avg)
            J.region_avg[region * 2 + t] = (uint8_t)((sum + (area >> 3)) / (area >> 2));
        if (J.total)
            atomicAdd(&J.total[t], sum);
    }
    if (region == 0 && J.region_avg && t >= regions_w * regions_h * 2 && t < 128) /* the padding of the picture's 128 bytes */
        J.region_avg[t] = 0;
}

/* ---------------------------------------------------------------- picture detectors ---------------------------------------------------------------- */

/* contextPtr->grad[lcu][5 + k] (:3551-3594): y / cr / cb point at the means of the sixteen 16x16 units */
__device__ __forceinline__ uint32_t detect_grad16(const uint8_t *y, const uint8_t *cr, const uint8_t *cb, int k)
{
    const int x = k & 3, r = k >> 2;
    int gx = 0, gy = 0, nx = 0, ny = 0;
#define DETECT_ABS3(i, j) (abs((int)y[i] - (int)y[j]) + abs((int)cr[i] - (int)cr[j]) + abs((int)cb[i] - (int)cb[j]))
    if (x != 0)
        gx += DETECT_ABS3(k, k - 1), nx++;
    if (x != 3)
        gx += DETECT_ABS3(k + 1, k), nx++;
    if (r != 0)
        gy += DETECT_ABS3(k, k - 4), ny++;
    if (r != 3)
        gy += DETECT_ABS3(k + 4, k), ny++;
#undef DETECT_ABS3
    return (uint32_t)(gx / nx + gy / ny) & 0xFFFFu;
}

__global__ __launch_bounds__(64) void k_detect_lcu(const DetectJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    const DetectJobDev &J = jobs[blockIdx.y];
    const int lcu = blockIdx.x, b = threadIdx.x, col = lcu % lcus_w, row = lcu / lcus_w, lx = col * 64, ly = row * 64;
    const SvtAmdPaLcuStats &S = J.stats[lcu];
    SvtAmdPaLcuDetect &o = J.lcu[lcu];
    const bool complete = lx + 64 <= width && ly + 64 <= height;
    const uint32_t v64 = S.variance[0];
    /* DetermineHomogeneousRegionInPicture: lane b holds the variance of 8x8 block b (raster); the 32x32 it belongs to: bits 0, 1 (x) and 3, 4 (y) */
    const unsigned long long v = S.variance[21 + b];
    unsigned long long sq = v * v, m = v;
    sq += __shfl_xor(sq, 1), m += __shfl_xor(m, 1);
    sq += __shfl_xor(sq, 2), m += __shfl_xor(m, 2);
    sq += __shfl_xor(sq, 8), m += __shfl_xor(m, 8);
    sq += __shfl_xor(sq, 16), m += __shfl_xor(m, 16);
    if (!(b & 27))
        o.var_of_var_32x32[((b >> 5) << 1) + ((b & 7) >> 2)] = complete ? (sq >> 4) - (m >> 4) * (m >> 4) : ~0ull; /* unsigned, as written (:3810) */
    sq += __shfl_xor(sq, 4), m += __shfl_xor(m, 4);
    sq += __shfl_xor(sq, 32), m += __shfl_xor(m, 32);
    const unsigned long long vov64 = (sq >> 6) - (m >> 6) * (m >> 6);
    /* sharpEdgeLcuFlag (:3683-3692): LCUs with a neighbour on every side */
    const bool interior = col > 0 && col < lcus_w - 1 && row > 0 && row < lcus_h - 1;
    const unsigned long long low16 = __ballot(b < 16 && S.variance[5 + b] < 20);
    /* EdgeDetectionMeanLumaChroma16x16, first loop: the gradients of complete potentialLogoLcu LCUs feed the picture's maxGrad */
    uint32_t grad = 0;
    if (J.chroma && complete && detect_logo_lcu(lx, ly, width, height, J.logo_cols, J.logo_rows)) { /* wave-uniform */
        if (b < 16)
            grad = detect_grad16(S.y_mean + 5, J.chroma[lcu].cr_mean + 5, J.chroma[lcu].cb_mean + 5, b);
        for (int s = 8; s > 0; s >>= 1)
            grad = max(grad, (uint32_t)__shfl_xor(grad, s));
    }
    if (b == 0) {
        o.edge_cu = 0, o.edge_block_num = 0, o.isolated_high_intensity = 0; /* k_detect_edge's and k_detect_finish's */
        o.homogeneous = !(complete && vov64 > 64 * 64);                     /* VAR_BASED_DETAIL_PRESERVATION_SELECTOR_THRSLHD */
        o.sharp_edge = interior && v64 > 200 && __popcll(low16) > 4;
#pragma unroll
        for (int i = 0; i < 10; i++)
            o.pad[i] = 0;
        atomicAdd(&J.red->var_sum, (unsigned long long)v64);
        if (complete && v64 < 5) /* LCU_LOW_VAR_TH */
            atomicAdd(&J.red->low_var, 1u);
        if (grad > 1)
            atomicMax(&J.red->max_grad, grad);
    }
}

/* picAvgVariance: the sum of the 64x64 variances of ALL LCUs / the LCU count, (EB_U16) (:3933) */
__device__ __forceinline__ uint32_t detect_pic_avg(const DetectReduce &R, int lcus) { return (uint32_t)(R.var_sum / (unsigned long long)lcus) & 0xFFFFu; }

/* grid (LCUs / 4, pictures): one wave per LCU, lanes 0..15 = the 16x16 units */
__global__ __launch_bounds__(256) void k_detect_edge(const DetectJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    const DetectJobDev &J = jobs[blockIdx.y];
    const int lcu = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), b = threadIdx.x & 63, lcus = lcus_w * lcus_h;
    if (lcu >= lcus)
        return;
    const int col = lcu % lcus_w, row = lcu / lcus_w;
    const SvtAmdPaLcuStats &S = J.stats[lcu];
    const uint32_t max_grad = max(J.red->max_grad, 1u);
    /* EdgeDetectionMeanLumaChroma16x16, second loop (:3602-3612) */
    bool edge = false;
    if (J.chroma && col * 64 + 64 <= width && row * 64 + 64 <= height && detect_logo_lcu(col * 64, row * 64, width, height, J.logo_cols, J.logo_rows) && b < 16)
        edge = min(detect_grad16(S.y_mean + 5, J.chroma[lcu].cr_mean + 5, J.chroma[lcu].cb_mean + 5, b) * 765u / max_grad, 255u) >= 30u;
    const unsigned long long edges = __ballot(edge);
    if (b == 0) {
        /* edgeBlockNum (:3680-3682): LCUs with a neighbour on every side, the 64x64 variance above 70 % of picAvgVariance */
        const bool interior = col > 0 && col < lcus_w - 1 && row > 0 && row < lcus_h - 1;
        const uint32_t ebn = interior && S.variance[0] > detect_pic_avg(*J.red, lcus) * 70u / 100u;
        SvtAmdPaLcuDetect &o = J.lcu[lcu];
        o.edge_cu = (uint16_t)edges, o.edge_block_num = (uint8_t)ebn;
        if (ebn)
            atomicAdd(&J.red->edge_lcus, 1u);
    }
}

/* grid (pictures), a workgroup per picture; dynamic LDS: mean[lcus], trigger[lcus] */
__global__ __launch_bounds__(256) void k_detect_finish(const DetectJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    extern __shared__ uint8_t lds[];
    const DetectJobDev &J = jobs[blockIdx.x];
    const int t = threadIdx.x, lcus = lcus_w * lcus_h;
    uint8_t *mean = lds, *trig = lds + lcus;
    for (int n = t; n < lcus; n += 256)
        mean[n] = J.stats[n].y_mean[0];
    __syncthreads();
    /* the LCUs that mark their 9x9 neighbourhood (:3696-3731): four LCUs on every side, mean above 180, a 4-neighbour below 120 */
    for (int n = t; n < lcus; n += 256) {
        const int col = n % lcus_w, row = n / lcus_w;
        trig[n] = col > 3 && col < lcus_w - 4 && row > 3 && row < lcus_h - 4 && mean[n] > 180 &&
                  (mean[n - 1] < 120 || mean[n + 1] < 120 || mean[n - lcus_w] < 120 || mean[n + lcus_w] < 120);
    }
    __syncthreads();
    for (int n = t; n < lcus; n += 256) {
        const int col = n % lcus_w, row = n / lcus_w;
        /* the final state of the raster loop: a mark survives on n only when its trigger m >= n */
        uint32_t iso = 0;
        for (int r = max(row, 4); r <= min(row + 4, lcus_h - 5); r++)
            for (int c = max(col - 4, 4); c <= min(col + 4, lcus_w - 5); c++)
                iso |= (r * lcus_w + c >= n) & trig[r * lcus_w + c];
        J.lcu[n].isolated_high_intensity = (uint8_t)iso;
    }
    if (t == 0) {
        const DetectReduce R = *J.red;
        const unsigned long long complete = (unsigned long long)(width / 64) * (unsigned long long)(height / 64); /* varLcuCnt */
        const unsigned long long pct = complete ? (unsigned long long)R.low_var * 100 / complete : 0;
        SvtAmdPaPicDetect p;
        p.pic_avg_variance = (uint16_t)detect_pic_avg(R, lcus);
        p.very_low_var_pic = pct > 60; /* PIC_LOW_VAR_PERCENTAGE_TH */
        p.logo_pic = pct > 80;
        p.lcu_block_percentage = (uint8_t)(R.edge_lcus * 100u / (uint32_t)lcus);
        p.pad[0] = p.pad[1] = p.pad[2] = 0;
        *J.pic = p;
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

extern "C" size_t svt_amd_chroma_stats_bytes(uint16_t luma_width, uint16_t luma_height, int which, int regions_w, int regions_h)
{
    const size_t lcus = (size_t)svt_amd_lcu_count(luma_width, luma_height);
    switch (which) {
    case SVT_AMD_CHROMA_MEANS:
        return lcus * sizeof(SvtAmdPaLcuChroma);
    case SVT_AMD_CHROMA_HISTOGRAM:
        return svt_amd_regions_ok(regions_w, regions_h) ? (size_t)regions_w * regions_h * 2 * 256 * sizeof(uint32_t) : 0;
    case SVT_AMD_CHROMA_REGION_AVG:
        return 128;
    case SVT_AMD_CHROMA_SUM:
        return 2 * sizeof(uint64_t);
    }
    return 0;
}

extern "C" size_t svt_amd_picture_detect_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    const size_t lcus = (size_t)svt_amd_lcu_count(luma_width, luma_height);
    switch (which) {
    case SVT_AMD_DETECT_LCU:
        return lcus * sizeof(SvtAmdPaLcuDetect);
    case SVT_AMD_DETECT_PICTURE:
        return sizeof(SvtAmdPaPicDetect);
    }
    return 0;
}

extern "C" int svt_amd_chroma_stats_batch_launch(SvtAmdContext *ctx, const SvtAmdChromaJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                 int regions_w, int regions_h, const SvtAmdChromaArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    const int w = luma_width, h = luma_height;
    if (w < 2 || h < 2 || (w & 1) || (h & 1))
        SVT_AMD_BAD("%s: job 0: a 4:2:0 picture of %dx%d", __func__, w, h);
    const int wl = (w + 63) / 64, lcus = svt_amd_lcu_count(w, h);
    bool any_means = false, any_hist = false;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdChromaJob &j = jobs[i];
        if (!j.want_means && !j.want_histogram)
            continue;
        if (!j.cb || !j.cr)
            SVT_AMD_BAD("%s: job %d wants chroma statistics, but has no %s plane", __func__, i, j.cb ? "Cr" : "Cb");
        if (j.pitch < (uint32_t)(w / 2) || j.pitch > 0x7FFFFFFFu)
            SVT_AMD_BAD("%s: job %d: a pitch of %u bytes for %d chroma samples a row", __func__, i, j.pitch, w / 2);
        if (j.want_means && !out->means)
            SVT_AMD_BAD("%s: job %d wants block means, but there is no means array", __func__, i);
        if (j.want_histogram && !out->histogram)
            SVT_AMD_BAD("%s: job %d wants histograms, but there is no histogram array", __func__, i);
        if (j.want_histogram && (!svt_amd_regions_ok(regions_w, regions_h) || w / regions_w < 8 || h / regions_h < 8))
            SVT_AMD_BAD("%s: job %d: %d x %d regions of a %dx%d picture", __func__, i, regions_w, regions_h, w, h);
        any_means |= j.want_means != 0;
        any_hist |= j.want_histogram != 0;
    }
    if (!any_means && !any_hist)
        return SVT_AMD_OK;
    const int regions = any_hist ? regions_w * regions_h : 0;

    ChromaJobDev *d_tab;
    unsigned long long *d_sums; /* the per-region sums the histogram kernels accumulate into */
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_CHROMA, sizeof(ChromaJobDev), CHROMA_SUMS_BYTES, (void **)&d_tab, (void **)&d_sums));
    const size_t b_hist = (size_t)regions * 2 * 256 * 4;
    static thread_local ChromaJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdChromaJob &j = jobs[i];
        ChromaJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        if (!j.want_means && !j.want_histogram)
            continue;
        d.cb = j.cb, d.cr = j.cr, d.pitch = (int32_t)j.pitch;
        d.means = j.want_means ? out->means + (size_t)i * lcus : nullptr;
        if (j.want_histogram) {
            d.hist = out->histogram + (size_t)i * regions * 2 * 256;
            d.sums = d_sums + (size_t)i * 128;
            d.region_avg = out->region_average ? out->region_average + (size_t)i * 128 : nullptr;
            d.total = out->sum_chroma ? (unsigned long long *)out->sum_chroma + (size_t)i * 2 : nullptr;
        }
    }
    /* the table goes up in stream order: a batch queued behind another one on this lane does not overwrite the table the first one still reads */
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(ChromaJobDev) * (size_t)num_jobs));
    if (any_hist) { /* what the histogram kernels accumulate into: one memset per run of pictures that want them */
        HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)num_jobs * 128 * 8, st));
        for (int i = 0, e; svt_amd_batch_run(&jobs[0].want_histogram, sizeof(jobs[0]), num_jobs, &i, &e); i = e) {
            HIP_TRY(hipMemsetAsync(out->histogram + (size_t)i * regions * 2 * 256, 0, (size_t)(e - i) * b_hist, st));
            if (out->sum_chroma)
                HIP_TRY(hipMemsetAsync(out->sum_chroma + (size_t)i * 2, 0, (size_t)(e - i) * 16, st));
        }
    }
    if (any_means)
        hipLaunchKernelGGL(k_chroma_means, dim3((unsigned)lcus, (unsigned)num_jobs), dim3(32), 0, st, (const ChromaJobDev *)d_tab, w, h, wl);
    if (any_hist) {
        hipLaunchKernelGGL(k_chroma_hist, dim3(CHROMA_STRIPS, (unsigned)regions, (unsigned)num_jobs), dim3(256), 0, st, (const ChromaJobDev *)d_tab, w, h, regions_w,
                           regions_h);
        hipLaunchKernelGGL(k_chroma_hist_finish, dim3((unsigned)regions, (unsigned)num_jobs), dim3(256), 0, st, (const ChromaJobDev *)d_tab, w, h, regions_w, regions_h);
    }
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

extern "C" int svt_amd_picture_detect_batch_launch(SvtAmdContext *ctx, const SvtAmdDetectJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                   const SvtAmdDetectArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    SvtAmdBatchGeometry g; /* no scratch per LCU: a picture larger than the context was made for is accepted */
    SVT_AMD_TRY(svt_amd_batch_geometry(__func__, ctx, luma_width, luma_height, DETECT_MAX_LCUS, false, &g));
    const auto [w, h, wl, hl, lcus, groups, cap_lcus, cap_groups] = g;
    if (!out->lcu || !out->picture)
        SVT_AMD_BAD("%s: job 0: there is no %s array", __func__, out->lcu ? "picture" : "lcu");
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdDetectJob &j = jobs[i];
        if (!j.stats)
            SVT_AMD_BAD("%s: job %d has no block statistics", __func__, i);
        if (j.want_edge16 && !j.chroma)
            SVT_AMD_BAD("%s: job %d wants the 16x16 edge map, but has no chroma means", __func__, i);
        if (j.resolution_class > 3)
            SVT_AMD_BAD("%s: job %d: resolution class %d", __func__, i, j.resolution_class);
    }

    DetectJobDev *d_tab;
    DetectReduce *d_red; /* the per-picture reduction the per-LCU kernel accumulates into */
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_DETECT, sizeof(DetectJobDev), DETECT_RED_BYTES, (void **)&d_tab, (void **)&d_red));
    static thread_local DetectJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdDetectJob &j = jobs[i];
        DetectJobDev &d = tab[i];
        d.stats = j.stats;
        d.chroma = j.want_edge16 ? j.chroma : nullptr;
        d.lcu = out->lcu + (size_t)i * lcus;
        d.pic = out->picture + i;
        d.red = d_red + i;
        /* INPUT_SIZE_576p_RANGE_OR_LOWER: 3 x 2 LCUs; below INPUT_SIZE_4K_RANGE: 7 x 4; 4K: 14 x 8 */
        d.logo_cols = svt_amd_logo_cols(j.resolution_class);
        d.logo_rows = svt_amd_logo_rows(j.resolution_class);
    }
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(DetectJobDev) * (size_t)num_jobs));
    /* the stages are ordered on the lane: a batch queued behind this one zeroes the reduction only after this one's finish kernel has read it */
    HIP_TRY(hipMemsetAsync(d_red, 0, sizeof(DetectReduce) * (size_t)num_jobs, st));
    hipLaunchKernelGGL(k_detect_lcu, dim3((unsigned)lcus, (unsigned)num_jobs), dim3(64), 0, st, (const DetectJobDev *)d_tab, w, h, wl, hl);
    hipLaunchKernelGGL(k_detect_edge, dim3((unsigned)((lcus + 3) / 4), (unsigned)num_jobs), dim3(256), 0, st, (const DetectJobDev *)d_tab, w, h, wl, hl);
    hipLaunchKernelGGL(k_detect_finish, dim3((unsigned)num_jobs), dim3(256), 2 * (size_t)lcus, st, (const DetectJobDev *)d_tab, w, h, wl, hl);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
