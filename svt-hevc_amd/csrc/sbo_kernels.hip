/*
 * sbo_kernels.hip - SourceBasedOperationsKernel (Codec/EbSourceBasedOperationsProcess.c:1397) and the two steps in front of it that feed it
 * (EbHevcUpdateBeaInfoOverTime, Codec/EbInitialRateControlProcess.c:519; DeriveSimilarCollocatedFlag, Codec/EbMotionEstimationProcess.c:462) in the batched,
 * stream-ordered shape of detect_kernels.hip (include/svt_hevc_amd.h "Batched source-based operations"): the picture is a grid dimension, the
 * per-picture pointers come from a descriptor table in device memory, nothing is copied to the host.  Integer logic on records; no plane is read.
 *   k_sbo_lcu       grid (LCUs / 4, pictures), a wave per LCU.  Lanes 0..15 = the 16x16 units (GrassSkinLcu :427, SpatialHighContrastClassifier :768); lanes 0..20
 *                   = the 64x64 / 32x32 / 16x16 units of the ME / OIS records, then a lane per 8x8 unit (QpmGatherStatistics :999; FailingMotionLcu :169,
 *                   DetectUncoveredLcu :228, TemporalHighContrastClassifier :741, ComplexityClassifier32x32 :120, LumaContrastDetectorLcu :364 on lanes 0..4);
 *                   the zz window and the similarity test are wave-uniform.  It STORES the LCU's record, a flag byte per LCU and - with want_qpm - one
 *                   28-word partial per workgroup (the four waves merged in LDS) into context-owned scratch: nothing is accumulated in memory, so nothing
 *                   has to be zeroed and a batch queued behind another one on the lane simply overwrites it.
 *   k_sbo_finish    grid (pictures), a workgroup of 512 threads per picture.  It reduces the flag bytes, the records' zz values and the QPM partials in LDS, then runs what needs
 *                   the reduced values or the 3x3 neighbourhood (lcuCmplxContrastArray in gather form, DetermineIsolatedNonHomogeneousRegionInPicture :536,
 *                   DetermineMorePotentialAuraAreas :639, DeriveBlockinessPresentFlag :958) with two bytes per LCU in LDS, and writes the picture record.
 * Bound: latency - 24 B written and a few hundred bytes touched per LCU (without want_qpm), 85 + 85 scattered words of the ME / OIS records with it.
 */
#include "pa_batch.h"
#include <string.h>

struct SboJobDev {
    const SvtAmdPaLcuStats *stats, *ref_stats;
    const SvtAmdPaLcuChroma *chroma;
    const SvtAmdPaLcuDetect *detect;
    const uint32_t *hist;
    const SvtAmdZzLcu *zz[17];
    const SvtAmdMeLcuResult *me;   /* null: no rule of this picture reads it */
    const SvtAmdOisLcuResult *ois;
    SvtAmdSboLcu *lcu;
    SvtAmdSboPic *pic;
    uint32_t *part;                /* [workgroups of k_sbo_lcu][SBO_PART_WORDS]: context-owned scratch */
    uint8_t *flags;                /* [lcus]: SBO_F_*, context-owned scratch */
    uint8_t zz_count, slice_type, layer, is_ref, res_class, skip8, cu8x8_mode, want_qpm;
};
static_assert(sizeof(SboJobDev) == 232, "SboJobDev layout");
static_assert(sizeof(SvtAmdSboJob) == 208 && sizeof(SvtAmdSboLcu) == 24 && sizeof(SvtAmdSboPic) == 168, "source-ops records");
#define SBO_MAX_LCUS 16384
#define SBO_PART_WORDS 32          /* 4 depths x (intra min, max, sum, inter min, max, sum, count), padded to 128 bytes */
#define SBO_F_TRIGGER 1            /* highContrastNum && highDist of a complete LCU (:1513) */
#define SBO_F_GRASS 2              /* lcuGrassFlag (:478) */
#define SBO_F_INTRA 4              /* cuOisSAD < cuMeSAD (:393) */
#define SBO_F_DEPTH1 8             /* depth1BlockNum counts this LCU (:394) */
/* k_sbo_finish's LDS bits per LCU */
#define SBO_L_TRIGGER 1
#define SBO_L_VAR_HIGH 2           /* variance[lcu][0] > IS_COMPLEX_LCU_VARIANCE_TH (100) */
#define SBO_L_VAR_MED 4            /* variance[lcu][0] <= MEDIUM_LCU_VARIANCE (50) */
#define SBO_L_HOMOGENEOUS 8        /* lcuHomogeneousAreaArray[lcu] == EB_TRUE */
#define SBO_L_EDGE_BLOCK 16        /* edgeResultsPtr[lcu].edgeBlockNum != 0 */

__device__ __forceinline__ uint32_t sbo_wave_min(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t sbo_wave_max(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t sbo_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += (uint32_t)__shfl_xor(v, o);
    return v;
}

/* min / max / sum / count of the lanes with `in` set, into seven words of the wave's partial in LDS */
__device__ __forceinline__ void sbo_qpm_depth(uint32_t *o, bool in, uint32_t ois, uint32_t me)
{
    const uint32_t i_min = sbo_wave_min(in ? ois : ~0u), i_max = sbo_wave_max(in ? ois : 0u), i_sum = sbo_wave_sum(in ? ois : 0u);
    const uint32_t e_min = sbo_wave_min(in ? me : ~0u), e_max = sbo_wave_max(in ? me : 0u), e_sum = sbo_wave_sum(in ? me : 0u);
    const uint32_t count = (uint32_t)__popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0)
        o[0] = i_min, o[1] = i_max, o[2] = i_sum, o[3] = e_min, o[4] = e_max, o[5] = e_sum, o[6] = count;
}

/* meToOisSadDeviation (:211-212, :278-279): the (EB_S32) casts, their 32-bit difference and the division as written */
__device__ __forceinline__ long long sbo_deviation(uint32_t me, unsigned long long ois)
{
    const long long diff = (int32_t)(me - (uint32_t)ois);
    return ois == 0 || diff < 0 ? 0 : (long long)((unsigned long long)(diff * 100) / ois);
}

/* grid (LCUs / 4, pictures): one wave per LCU */
__global__ __launch_bounds__(256) void k_sbo_lcu(const SboJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus)
{
    __shared__ uint32_t s_part[4][28];
    const SboJobDev &J = jobs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int lcu = (int)blockIdx.x * 4 + wave;
    const bool active = lcu < lcus;
    const int n = active ? lcu : lcus - 1; /* a wave past the last LCU computes the last one again and stores nothing */
    const int col = n % lcus_w, row = n / lcus_w, ox = col * 64, oy = row * 64;
    const bool complete = ox + 64 <= width && oy + 64 <= height;
    const int slice = J.slice_type, layer = J.layer;
    const SvtAmdPaLcuStats &S = J.stats[n];

    /* EbHevcUpdateBeaInfoOverTime: the window's sums / the window's length, (EB_U8); EbHevcInitZzCostInfo without a window */
    uint32_t zz_sum = 0, nm_sum = 0;
    if (J.zz_count) { /* all seventeen loads in flight at once: a slot past the window reads record 0 again and adds nothing */
#pragma unroll
        for (int i = 0; i < 17; i++) {
            const SvtAmdZzLcu z = J.zz[i < J.zz_count ? i : 0][n];
            zz_sum += i < J.zz_count ? z.zz_cost : 0u, nm_sum += i < J.zz_count ? z.non_moving_index : 0u;
        }
    }
    const uint32_t zz_cost = J.zz_count ? (zz_sum / J.zz_count) & 0xFFu : 0xFFu, non_moving = J.zz_count ? (nm_sum & 0xFFFFu) / J.zz_count & 0xFFu : 0xFFu;

    /* DeriveSimilarCollocatedFlag */
    bool similar_all = false;
    if (slice != 0 && J.ref_stats) {
        const long long ref_mean = J.ref_stats[n].y_mean[0], ref_var = max((int)J.ref_stats[n].variance[0], 1);
        const long long cur_mean = S.y_mean[0], cur_var = S.variance[0];
        similar_all = llabs(cur_mean - ref_mean) < 10 && (llabs(cur_var * 100 / ref_var - 100) < 10 || llabs(cur_var - ref_var) < 10);
    }
    const bool similar = similar_all && J.is_ref;

    /* GrassSkinLcu and SpatialHighContrastClassifier: lane k = 16x16 unit k */
    bool grass = false, skin = false, high_luma = false, high_chroma = false, contrast = false;
    if (b < 16) {
        const int y = S.y_mean[5 + b], cb = J.chroma[n].cb_mean[5 + b], cr = J.chroma[n].cr_mean[5 + b], var = S.variance[5 + b];
        if (ox + (b & 3) * 16 + 16 <= width && oy + (b >> 2) * 16 + 16 <= height) { /* rasterScanCuValidity */
            grass = y > 70 && y < 130 && cb > 80 && cb < 115 && cr > 110 && cr < 135;
            skin = y > 52 && y < 130 && cb > 100 && cb < 120 && cr > 135 && cr < 160;
            high_chroma = cr >= 127 || cb > 150;
            high_luma = cr >= 80 && y > 180;
        }
        contrast = var > 10 && var < 300 && y > 70 && y < 145 && abs(cb - 140) < 10 && abs(cr - 115) < 15;
    }
    const uint32_t m_grass = (uint32_t)__ballot(grass), m_skin = (uint32_t)__ballot(skin), m_luma = (uint32_t)__ballot(high_luma),
                   m_chroma = (uint32_t)__ballot(high_chroma);
    const bool high_contrast = __ballot(contrast) != 0;

    /* the ME / OIS records: lanes 0..20 = the 64x64, 32x32 and 16x16 units by rasterScanCuIndex, then every lane its 8x8 unit */
    bool failing = false, uncovered = false, high_dist = false, noise = false, intra = false;
    const bool read_records = slice != 0 || J.want_qpm; /* the host made sure that both tables are there */
    uint32_t me2 = 0, ois2 = 0, ois_w2 = 0;
    unsigned long long ois64 = 0;
    if (read_records) {
        const SvtAmdMeLcuResult &M = J.me[n];
        const SvtAmdOisLcuResult &O = J.ois[n];
        if (b < 21)
            me2 = M.pu[b].distortion[0], ois_w2 = b ? O.candidate[b][0] : 0u;
        ois2 = ois_w2 & 0xFFFFFu;
        ois64 = (unsigned long long)__shfl(ois2, 1) + __shfl(ois2, 2) + __shfl(ois2, 3) + __shfl(ois2, 4); /* the 64x64: the four 32x32 (:200-203) */
        if (slice != 0) {
            const long long dev = b < 5 ? sbo_deviation(me2, b ? ois2 : ois64) : 0;
            failing = complete && !similar && __ballot(dev > 15) != 0;                        /* SAD_DEVIATION_LCU_TH_0 */
            uncovered = layer == 0 && complete && !similar && __ballot(dev > 20) != 0;        /* SAD_DEVIATION_LCU_TH_1 */
            intra = ois64 < __shfl(me2, 0);
        }
        if (slice == 2) {
            const uint32_t nsad = b >= 1 && b < 5 ? me2 >> 10 : 0u;
            high_dist = __ballot(b >= 1 && b < 5 && nsad >= (layer == 0 ? 10u : 5u)) != 0;    /* nsadTable (:748) */
            const uint32_t th = layer == 0 ? 33u : layer == 1 ? 28u : layer == 2 ? 27u : 26u;  /* THRESHOLD_NOISE (:53) */
            noise = layer >= 1 && complete && __ballot(b >= 1 && b < 5 && nsad > th) != 0;
        }
        if (J.want_qpm) { /* QpmGatherStatistics: workgroup-uniform */
            uint32_t *part = s_part[wave];
            const bool v64 = b == 0 && complete;
            const bool v32 = b >= 1 && b < 5 && ox + ((b - 1) & 1) * 32 + 32 <= width && oy + ((b - 1) >> 1) * 32 + 32 <= height;
            const bool v16 = b >= 5 && b < 21 && ox + ((b - 5) & 3) * 16 + 16 <= width && oy + ((b - 5) >> 2) * 16 + 16 <= height;
            sbo_qpm_depth(part + 0, active && v64, (uint32_t)ois64, me2);
            sbo_qpm_depth(part + 7, active && v32, ois2, me2);
            sbo_qpm_depth(part + 14, active && v16, ois2, me2);
            const int bx = b & 7, by = b >> 3;
            const uint32_t parent = __shfl(ois_w2, 5 + (by >> 1) * 4 + (bx >> 1));
            const uint32_t w8 = O.candidate[21 + b][0];
            const uint32_t ois8 = J.cu8x8_mode == 0 && (w8 >> 20 & 1u) ? w8 & 0xFFFFFu : (parent >> 20 & 1u) ? parent & 0xFFFFFu : 0u;
            const bool v8 = !J.skip8 && ox + bx * 8 + 8 <= width && oy + by * 8 + 8 <= height;
            sbo_qpm_depth(part + 21, active && v8, ois8, M.pu[21 + b].distortion[0]);
        }
    }
    if (J.want_qpm) {
        __syncthreads();
        const int t = threadIdx.x;
        if (t < 28) {
            const int k = t % 7;
            uint32_t v = s_part[0][t];
            for (int i = 1; i < 4; i++)
                v = k == 0 || k == 3 ? min(v, s_part[i][t]) : k == 1 || k == 4 ? max(v, s_part[i][t]) : v + s_part[i][t];
            J.part[(size_t)blockIdx.x * SBO_PART_WORDS + t] = v;
        }
    }
    if (active && b == 0) {
        SvtAmdSboLcu o;
        o.grass = (uint16_t)m_grass, o.skin = (uint16_t)m_skin, o.high_luma = (uint16_t)m_luma, o.high_chroma = (uint16_t)m_chroma;
        o.zz_cost = (uint8_t)zz_cost, o.non_moving_index = (uint8_t)non_moving;
        o.similar_colocated = similar, o.similar_colocated_all_layers = similar_all;
        o.failing_motion = failing, o.uncovered_area = uncovered;
        o.cmplx_contrast = 0, o.isolated_non_homogeneous = 0, o.complex_lcu = 0; /* k_sbo_finish's */
        o.cmplx_status = noise ? 4 : 0;
#pragma unroll
        for (int i = 0; i < 6; i++)
            o.pad[i] = 0;
        J.lcu[n] = o;
        const bool depth1 = complete && slice != 0 && layer == 0; /* LumaContrastDetectorLcu */
        J.flags[n] = (uint8_t)((complete && high_contrast && high_dist ? SBO_F_TRIGGER : 0) | (m_grass ? SBO_F_GRASS : 0) | (depth1 && intra ? SBO_F_INTRA : 0) |
                               (depth1 ? SBO_F_DEPTH1 : 0));
    }
}

#define SBO_FINISH_THREADS 512
#define SBO_FINISH_WAVES (SBO_FINISH_THREADS / 64)
#define SBO_FINISH_STRIDES (SBO_FINISH_THREADS / SBO_PART_WORDS)

/* the sum over the workgroup's threads; every thread gets it.  red: SBO_FINISH_WAVES words of LDS nobody else uses */
__device__ __forceinline__ uint32_t sbo_block_sum(uint32_t v, uint32_t *red)
{
    v = sbo_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < SBO_FINISH_WAVES; i++)
        sum += red[i];
    return sum;
}

/* grid (pictures), a workgroup of 512 threads per picture; dynamic LDS: 16 x 32 words of the QPM reduction + 8 words, then non_moving[lcus], bits[lcus] */
#define SBO_FINISH_LDS_WORDS (SBO_FINISH_STRIDES * SBO_PART_WORDS + SBO_FINISH_WAVES)
__global__ __launch_bounds__(SBO_FINISH_THREADS) void k_sbo_finish(const SboJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h, int regions)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const SboJobDev &J = jobs[blockIdx.x];
    const int t = threadIdx.x, lcus = lcus_w * lcus_h;
    uint32_t *qred = (uint32_t *)lds, *red = qred + SBO_FINISH_STRIDES * SBO_PART_WORDS;
    uint8_t *nmi = lds + SBO_FINISH_LDS_WORDS * 4, *bits = nmi + lcus;

    uint32_t nm_sum = 0, zz_sum = 0, grass = 0, moving = 0, moving_n = 0, still = 0, still_n = 0, intra = 0, depth1 = 0;
    for (int n = t; n < lcus; n += SBO_FINISH_THREADS) {
        const int col = n % lcus_w, row = n / lcus_w;
        const bool complete = col * 64 + 64 <= width && row * 64 + 64 <= height;
        const uint32_t nm = J.lcu[n].non_moving_index, f = J.flags[n], var = J.stats[n].variance[0], mean = J.stats[n].y_mean[0];
        nmi[n] = (uint8_t)nm;
        bits[n] = (uint8_t)((f & SBO_F_TRIGGER ? SBO_L_TRIGGER : 0) | (var > 100 ? SBO_L_VAR_HIGH : 0) | (var <= 50 ? SBO_L_VAR_MED : 0) |
                            (J.detect[n].homogeneous == 1 ? SBO_L_HOMOGENEOUS : 0) | (J.detect[n].edge_block_num ? SBO_L_EDGE_BLOCK : 0));
        if (complete)
            nm_sum += nm, zz_sum += J.lcu[n].zz_cost;
        grass += f & SBO_F_GRASS ? 1 : 0, intra += f & SBO_F_INTRA ? 1 : 0, depth1 += f & SBO_F_DEPTH1 ? 1 : 0;
        if (nm < 10)
            still += mean, still_n++;
        else
            moving += mean, moving_n++;
    }
    /* DeriveHighDarkAreaDensityFlag: thread t = bin t & 255 of every (t >> 8)th region; 32-bit sums as written */
    uint32_t bin = 0;
    for (int r = t >> 8; r < regions; r += SBO_FINISH_THREADS / 256)
        bin += J.hist[r * 256 + (t & 255)];
    const uint32_t black25 = sbo_block_sum((t & 255) < 25 ? bin : 0u, red), black40 = sbo_block_sum((t & 255) < 40 ? bin : 0u, red),
                   white = sbo_block_sum((t & 255) >= 210 ? bin : 0u, red);
    nm_sum = sbo_block_sum(nm_sum, red), zz_sum = sbo_block_sum(zz_sum, red), grass = sbo_block_sum(grass, red);
    moving = sbo_block_sum(moving, red), moving_n = sbo_block_sum(moving_n, red), still = sbo_block_sum(still, red), still_n = sbo_block_sum(still_n, red);
    intra = sbo_block_sum(intra, red), depth1 = sbo_block_sum(depth1, red);
    /* DerivePictureActivityStatistics; with no complete LCU the averages are 0 */
    const uint32_t complete_n = (uint32_t)(width / 64) * (uint32_t)(height / 64);
    const uint32_t nm_avg = complete_n ? nm_sum / complete_n & 0xFFFFu : 0u, zz_avg = complete_n ? zz_sum / complete_n : 0u;

    if (J.want_qpm) { /* the workgroups' partials: thread = (word, one of SBO_FINISH_STRIDES strides) */
        const int k = t & 31, groups = (lcus + 3) / 4, op = k % 7;
        uint32_t v = op == 0 || op == 3 ? ~0u : 0u;
        if (k < 28)
            for (int g = t >> 5; g < groups; g += SBO_FINISH_STRIDES) {
                const uint32_t p = J.part[(size_t)g * SBO_PART_WORDS + k];
                v = op == 0 || op == 3 ? min(v, p) : op == 1 || op == 4 ? max(v, p) : v + p;
            }
        qred[t] = v;
    }
    __syncthreads(); /* nmi, bits and qred are complete */
    if (J.want_qpm && t < 28) { /* word t over the strides, left in the first row: thread 0 reads it behind the barriers of the last sum below */
        const int op = t % 7;
        uint32_t v = qred[t];
        for (int s = 1; s < SBO_FINISH_STRIDES; s++) {
            const uint32_t q = qred[s * SBO_PART_WORDS + t];
            v = op == 0 || op == 3 ? min(v, q) : op == 1 || op == 4 ? max(v, q) : v + q;
        }
        qred[t] = v;
    }

    uint32_t aura = 0;
    for (int n = t; n < lcus; n += SBO_FINISH_THREADS) {
        const int col = n % lcus_w, row = n / lcus_w, ox = col * 64, oy = row * 64;
        const bool left = col > 0, right = ox + 64 < width, top = row > 0, bottom = oy + 64 < height;
        /* lcuCmplxContrastArray after the raster loop: only a trigger m > n leaves its mark on n - n is the left, top, top-left or top-right neighbour of m,
         * whose populate conditions (:815, :825, :835, :840) hold for every such m inside the picture */
        const uint32_t contrast = (col + 1 < lcus_w && (bits[n + 1] & SBO_L_TRIGGER)) || (row + 1 < lcus_h && (bits[n + lcus_w] & SBO_L_TRIGGER)) ||
                                  (col + 1 < lcus_w && row + 1 < lcus_h && (bits[n + lcus_w + 1] & SBO_L_TRIGGER)) ||
                                  (col > 0 && row + 1 < lcus_h && (bits[n + lcus_w - 1] & SBO_L_TRIGGER));
        /* DetermineIsolatedNonHomogeneousRegionInPicture */
        uint32_t isolated = 0;
        if (col > 0 && col < lcus_w - 1 && row > 0 && row < lcus_h - 1) {
            const bool right_c = ox + 128 <= width, below_c = oy + 128 <= height; /* isCompleteLcu of the column to the right / the row below (:559-565) */
            const int up = n - lcus_w, dn = n + lcus_w;
            const int flat = ((bits[up - 1] & SBO_L_VAR_MED) ? 1 : 0) + ((bits[up] & SBO_L_VAR_MED) ? 1 : 0) + ((bits[up + 1] & SBO_L_VAR_MED) && right_c ? 1 : 0) +
                             ((bits[dn - 1] & SBO_L_VAR_MED) && below_c ? 1 : 0) + ((bits[dn] & SBO_L_VAR_MED) && below_c ? 1 : 0) +
                             ((bits[dn + 1] & SBO_L_VAR_MED) && below_c && right_c ? 1 : 0) + ((bits[n + 1] & SBO_L_VAR_MED) && right_c ? 1 : 0) +
                             ((bits[n - 1] & SBO_L_VAR_MED) ? 1 : 0);
            if (flat > 1) {
                bool nonhom = false;
                for (int q = 0; q < 4; q++)
                    nonhom |= J.detect[n].var_of_var_32x32[q] > 64 * 64;
                const int homog = ((bits[up - 1] & SBO_L_HOMOGENEOUS) ? 1 : 0) + ((bits[up + 1] & SBO_L_HOMOGENEOUS) ? 1 : 0) +
                                  ((bits[dn - 1] & SBO_L_HOMOGENEOUS) ? 1 : 0) + ((bits[dn + 1] & SBO_L_HOMOGENEOUS) ? 1 : 0);
                isolated = nonhom && homog >= 2;
            }
        }
        /* DeriveBlockinessPresentFlag: IsSpatiallyComplexArea counts the LCU itself as available only when its variance is high (:873) */
        int avail = 0, high = 0;
        if (bits[n] & SBO_L_VAR_HIGH)
            avail++, high++;
#define SBO_NEIGHBOUR(cond, at) \
    if (cond)                   \
        avail++, high += (bits[at] & SBO_L_VAR_HIGH) ? 1 : 0;
        SBO_NEIGHBOUR(left, n - 1)
        SBO_NEIGHBOUR(right, n + 1)
        SBO_NEIGHBOUR(top, n - lcus_w)
        SBO_NEIGHBOUR(bottom, n + lcus_w)
        SBO_NEIGHBOUR(left && top, n - lcus_w - 1)
        SBO_NEIGHBOUR(right && top, n - lcus_w + 1)
        SBO_NEIGHBOUR(left && bottom, n + lcus_w - 1)
        SBO_NEIGHBOUR(right && bottom, n + lcus_w + 1)
#undef SBO_NEIGHBOUR
        uint32_t complex_lcu = 0;
        if (high == avail && nmi[n] != 0xFF && nm_avg != 0xFF) {
            if (nmi[n] == 30 && nm_avg >= 29 && J.layer > 0 && J.res_class == 3)
                complex_lcu = 2;
            else if (nmi[n] == 30 && nm_avg >= 23 && nm_avg < 29)
                complex_lcu = 1;
        }
        /* DetermineMorePotentialAuraAreas: isEdgeLcu (Codec/EbSequenceControlSet.c:210); an index outside the array counts as 0 */
        if (!(ox < 64 || oy < 64 || ox > width - 64 || oy > height - 64) && (bits[n] & SBO_L_EDGE_BLOCK) && J.stats[n].y_mean[0] >= 150) {
            int quiet = 0;
            for (int v = -1; v <= 1; v++)
                for (int h = -1; h <= 1; h++) {
                    const int at = n + v * lcus_w + h;
                    quiet += at >= 0 && at < lcus && !(bits[at] & SBO_L_EDGE_BLOCK) && nmi[at] < 30;
                }
            aura += quiet > 1;
        }
        SvtAmdSboLcu &o = J.lcu[n];
        o.cmplx_contrast = (uint8_t)contrast, o.isolated_non_homogeneous = (uint8_t)isolated, o.complex_lcu = (uint8_t)complex_lcu;
    }
    aura = sbo_block_sum(aura, red);

    if (t == 0) {
        SvtAmdSboPic &p = *J.pic; /* every byte of the record is stored */
        p.complete_lcu_count = complete_n, p.zz_cost_average = zz_avg, p.non_moving_index_average = (uint16_t)nm_avg;
        p.low_motion_content = zz_avg == 0;
        /* LumaContrastDetectorPicture */
        const uint32_t still_mean = still_n ? still / still_n : 0u, moving_mean = moving_n ? moving / moving_n : 0u;
        p.dark_background_light_foreground = moving_mean > 2 * still_mean && still_mean < 45; /* DARK_FRM_TH */
        p.intra_coded_block_probability = J.slice_type != 0 && J.layer == 0 && depth1 ? (uint8_t)(intra * 100u / depth1) : 0;
        p.grass_percentage = (uint8_t)(grass * 100u / (uint32_t)lcus);
        p.percentage_of_edge_in_light_background = (uint8_t)(aura * 100u / (uint32_t)lcus);
        const uint32_t area = (uint32_t)(width * height);
        p.high_dark_area_density = black25 * 100u / area >= 20; /* MIN_BLACK_AREA_PERCENTAGE */
        p.black_area_percentage = (uint8_t)(black40 * 100u / area);
        p.high_dark_low_light_area_density = black40 * 100u / area >= 20 && white * 100u / area >= 1;
#pragma unroll
        for (int i = 0; i < 6; i++)
            p.pad[i] = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) { /* the picture part of the QPM statistics (:1585-1660); all zero without want_qpm */
            uint32_t imin = 0, imax = 0, iacc = 0, iavg = 0, emin = 0, emax = 0, eacc = 0, eavg = 0, leaves = 0;
            if (J.want_qpm) {
                const uint32_t *w = qred + d * 7;
                imin = w[0], imax = w[1], iacc = w[2], emin = w[3], emax = w[4], eacc = w[5], leaves = w[6];
                if (d < (J.skip8 ? 3 : 4) && leaves) {
                    iavg = iacc / leaves, eavg = eacc / leaves;
                    const int32_t i_lo = abs((int32_t)imin - (int32_t)iavg), i_hi = (int32_t)imax - (int32_t)iavg;
                    if (i_lo < i_hi)
                        imax = iavg + (uint32_t)i_lo;
                    else
                        imin = iavg - (uint32_t)i_hi;
                    int32_t e_lo = 0, e_hi = 0;
                    if (J.slice_type != 0)
                        e_lo = abs((int32_t)emin - (int32_t)eavg), e_hi = (int32_t)emax - (int32_t)eavg;
                    if (e_lo < e_hi)
                        emax = eavg + (uint32_t)e_lo;
                    else
                        emin = eavg - (uint32_t)e_hi;
                }
            }
            p.intra_complexity_min[d] = imin, p.intra_complexity_max[d] = imax, p.intra_complexity_accum[d] = iacc, p.intra_complexity_avg[d] = iavg;
            p.inter_complexity_min[d] = emin, p.inter_complexity_max[d] = emax, p.inter_complexity_accum[d] = eacc, p.inter_complexity_avg[d] = eavg;
            p.processed_leaf_count[d] = leaves;
        }
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

extern "C" size_t svt_amd_source_ops_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    switch (which) {
    case SVT_AMD_SBO_LCU:
        return (size_t)svt_amd_lcu_count(luma_width, luma_height) * sizeof(SvtAmdSboLcu);
    case SVT_AMD_SBO_PICTURE:
        return sizeof(SvtAmdSboPic);
    }
    return 0;
}

extern "C" int svt_amd_source_ops_batch_launch(SvtAmdContext *ctx, const SvtAmdSboJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                               int regions_w, int regions_h, const SvtAmdSboArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    SvtAmdBatchGeometry g;
    SVT_AMD_TRY(svt_amd_batch_geometry(__func__, ctx, luma_width, luma_height, SBO_MAX_LCUS, true, &g));
    const auto [w, h, wl, hl, lcus, groups, cap_lcus, cap_groups] = g;
    if (!out->lcu || !out->picture)
        SVT_AMD_BAD("%s: job 0: there is no %s array", __func__, out->lcu ? "picture" : "lcu");
    if (!svt_amd_regions_ok(regions_w, regions_h))
        SVT_AMD_BAD("%s: job 0: %d x %d regions", __func__, regions_w, regions_h);
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdSboJob &j = jobs[i];
        if (!j.stats || !j.chroma || !j.detect || !j.histogram)
            SVT_AMD_BAD("%s: job %d has no %s", __func__, i, !j.stats ? "block statistics" : !j.chroma ? "chroma means" : !j.detect ? "detector records" : "luma histogram");
        if (j.zz_count > 17)
            SVT_AMD_BAD("%s: job %d: a look-ahead window of %d pictures (at most 17)", __func__, i, j.zz_count);
        for (int k = 0; k < j.zz_count; k++)
            if (!j.zz[k])
                SVT_AMD_BAD("%s: job %d: zz[%d] of a window of %d pictures is NULL", __func__, i, k, j.zz_count);
        if (j.slice_type > 2 || j.temporal_layer_index > 5 || j.resolution_class > 3)
            SVT_AMD_BAD("%s: job %d: slice type %d, temporal layer %d, resolution class %d", __func__, i, j.slice_type, j.temporal_layer_index, j.resolution_class);
        if ((j.slice_type != 0 || j.want_qpm) && (!j.me || !j.ois)) /* the records resident in the slot */
            SVT_AMD_TRY(svt_amd_batch_slot_records(__func__, ctx, i, j.cur_slot, (j.me ? 0 : BATCH_REC_ME) | (j.ois ? 0 : BATCH_REC_OIS), w, h));
    }

    SboJobDev *d_tab;
    uint8_t *d_scratch; /* per picture: the workgroups' QPM partials, then a flag byte per LCU */
    const size_t pic_scratch = (size_t)cap_groups * SBO_PART_WORDS * 4 + (size_t)cap_groups * 4;
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_SBO, sizeof(SboJobDev), pic_scratch * SVT_AMD_MAX_BATCH, (void **)&d_tab, (void **)&d_scratch));
    static thread_local SboJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    SvtAmdRecordsBinder bind;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdSboJob &j = jobs[i];
        SboJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        d.stats = j.stats, d.ref_stats = j.ref_stats, d.chroma = j.chroma, d.detect = j.detect, d.hist = j.histogram;
        for (int k = 0; k < j.zz_count; k++)
            d.zz[k] = j.zz[k];
        if (j.slice_type != 0 || j.want_qpm) {
            d.me = j.me, d.ois = j.ois;
            if (!j.me)
                SVT_AMD_TRY(svt_amd_batch_bind_records(ctx, &bind, j.cur_slot, SLOT_ME, (const void **)&d.me));
            if (!j.ois)
                SVT_AMD_TRY(svt_amd_batch_bind_records(ctx, &bind, j.cur_slot, SLOT_OIS, (const void **)&d.ois));
        }
        d.lcu = out->lcu + (size_t)i * lcus;
        d.pic = out->picture + i;
        d.part = (uint32_t *)(d_scratch + (size_t)i * pic_scratch);
        d.flags = d_scratch + (size_t)i * pic_scratch + (size_t)cap_groups * SBO_PART_WORDS * 4;
        d.zz_count = j.zz_count, d.slice_type = j.slice_type, d.layer = j.temporal_layer_index, d.is_ref = j.is_used_as_reference != 0;
        d.res_class = j.resolution_class, d.skip8 = j.skip_ois_8x8 != 0, d.cu8x8_mode = j.cu8x8_mode, d.want_qpm = j.want_qpm != 0;
    }
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(SboJobDev) * (size_t)num_jobs));
    /* the stages are ordered on the lane, and the scratch is stored into, never added to: a batch queued behind this one overwrites it only after this one's
     * finish kernel has read it, and there is nothing to zero */
    hipLaunchKernelGGL(k_sbo_lcu, dim3((unsigned)groups, (unsigned)num_jobs), dim3(256), 0, st, (const SboJobDev *)d_tab, w, h, wl, lcus);
    hipLaunchKernelGGL(k_sbo_finish, dim3((unsigned)num_jobs), dim3(SBO_FINISH_THREADS), (size_t)SBO_FINISH_LDS_WORDS * 4 + 2 * (size_t)lcus, st, (const SboJobDev *)d_tab, w, h,
                       wl, hl, regions_w * regions_h);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
