/*
 * irc_kernels.hip - the look-ahead stage of InitialRateControlKernel (Codec/EbInitialRateControlProcess.c:849: EbHevcDetectGlobalMotion :218,
 * EbHevcUpdateGlobalMotionDetectionOverTime :441, EbHevcUpdateMotionFieldUniformityOverTime :598 with EbHevcStationaryEdgeCountLcu :394, UpdateHomogeneityOverTime
 * :646), the two per-LCU checks in front of it (StationaryEdgeOverUpdateOverTimeLcuPart1 / Part2, Codec/EbMotionEstimationProcess.c:502, :554) and the final
 * stationary-edge stage behind it (StationaryEdgeOverUpdateOverTimeLcu, Codec/EbSourceBasedOperationsProcess.c:1142) in the batched, stream-ordered shape of
 * sbo_kernels.hip / mdc_kernels.hip (include/svt_hevc_amd.h "Batched initial rate control"): the picture is a grid dimension, the per-picture
 * pointers come from a descriptor table in device memory, nothing is copied to the host.  Integer logic on records; no plane is read.  Restated as
 * tests/irc_numpy.py spells it out.  The look-ahead window is three lists of record pointers the caller has walked; an entry may be an array this very batch
 * writes, so every array is written by ONE kernel and a stage that reads another picture's record runs in a later launch than the stage that writes it.
 *   k_irc_lcu       grid (LCUs / 4, pictures), a wave per LCU.  Part1 / Part2 (wave-uniform); EbHevcDetectGlobalMotion's four tests: lanes 0..4 load the first
 *                   word - xMvL0, yMvL0 of the 64x64 unit - of the LCU's and its left, top, right and bottom neighbour's ME record, lanes 1..4 test their
 *                   neighbour against lane 0's vector, a vote is a ballot.  It STORES the checks, a vote byte per LCU and one word of vote totals per
 *                   workgroup (the four waves merged in LDS) into context-owned scratch: nothing is accumulated in memory, nothing has to be zeroed.
 *   k_irc_motion    grid (pictures), a workgroup of 256 threads per picture: the workgroups' totals into the motion record.
 *   k_irc_counts    grid (LCUs / 4, pictures), a wave per LCU, behind k_irc_lcu of EVERY picture.  Lanes 0..31 = a 16x16 unit and a flavour (plain, PM): the count
 *                   of the window entries whose own check holds and whose edge_cu bit is set; "at least 4 of 16 above the threshold" is a ballot and a
 *                   population count.  Lanes 32..47 = an entry of the homogeneity window: its 64x64 variance, wave sums.  The LCU's whole record, and a flag
 *                   byte per LCU into scratch.
 *   k_irc_finish    grid (pictures), a workgroup of 1024 threads per picture, behind k_irc_motion of EVERY picture.  The three 3x3 passes on both planes with one
 *                   byte per LCU (both flags and the gate of passes (b) / (c)) in LDS, ping-pong between two rows, one barrier a pass; pass (a) in its gather
 *                   form.  Pan over time, the homogeneity count, the picture record.
 * Bound: latency - under a hundred bytes written and a few hundred read per LCU, five scattered words of the ME records.
 */
#include "pa_batch.h"
#include <string.h>

struct IrcJobDev {
    const SvtAmdMeLcuResult *me;   /* null: no rule of this picture reads it */
    const SvtAmdPaLcuStats *stats;
    const SvtAmdIrcChecks *edge_checks[4];
    const SvtAmdPaLcuDetect *edge_detect[4];
    const SvtAmdPaLcuStats *hom_stats[16];
    const SvtAmdIrcMotion *pan_motion[8];
    SvtAmdIrcChecks *checks;
    SvtAmdIrcMotion *motion;
    SvtAmdIrcLcu *lcu;
    uint8_t *stationary, *pm_stationary;
    SvtAmdIrcPic *pic;
    uint32_t *part;                /* [workgroups of k_irc_lcu]: IRC_P_* totals, context-owned scratch */
    uint8_t *votes;                /* [lcus]: motion_votes, context-owned scratch */
    uint8_t *flags;                /* [lcus]: IRC_F_*, context-owned scratch */
    uint8_t edge_count, hom_count, pan_count, slice, layer, hier, cls, look_ahead, frames, pad[7];
};
static_assert(sizeof(IrcJobDev) == 360, "IrcJobDev layout");
static_assert(sizeof(SvtAmdIrcJob) == 288 && sizeof(SvtAmdIrcChecks) == 4 && sizeof(SvtAmdIrcMotion) == 24 && sizeof(SvtAmdIrcLcu) == 48 && sizeof(SvtAmdIrcPic) == 16,
              "initial rate control records");
static_assert(offsetof(SvtAmdIrcLcu, var_of_var_over_time) == 32 && offsetof(SvtAmdIrcLcu, motion_votes) == 41, "SvtAmdIrcLcu layout");
/* the vote byte: bit 0 pan, 1 tilt, 2 pan high amplitude, 3 tilt high amplitude; the workgroup's word: a 4-bit total (0..4) each, the checked LCUs lowest */
#define IRC_P_SHIFT 4
/* the flag byte of k_irc_counts */
#define IRC_F_EDGE 1               /* stationaryEdgeOverTimeFlag before the passes (:1168) */
#define IRC_F_PM_EDGE 2            /* pmStationaryEdgeOverTimeFlag before the passes (:1181) */
#define IRC_F_HOMOGENEOUS 4        /* isLcuHomogeneousOverTime */
/* k_irc_finish's LDS byte per LCU: bits 0-1 the flag, bits 2-3 the PM flag, bit 4 potentialLogoLcu && (check2 || !isCompleteLcu) */
#define IRC_L_GATE 16
#define IRC_MOTION_THREADS 256
#define IRC_FINISH_THREADS 1024

__device__ __forceinline__ uint32_t irc_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += (uint32_t)__shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long irc_wave_sum64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += (unsigned long long)__shfl_xor(v, o);
    return v;
}
/* the sum over the workgroup's threads; every thread gets it.  red: a word per wave of LDS nobody else uses */
template <int WAVES> __device__ __forceinline__ uint32_t irc_block_sum(uint32_t v, uint32_t *red)
{
    v = irc_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++)
        sum += red[i];
    return sum;
}

/* grid (LCUs / 4, pictures): one wave per LCU */
__global__ __launch_bounds__(256) void k_irc_lcu(const IrcJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus)
{
    __shared__ uint32_t s_part[4];
    const IrcJobDev &J = jobs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int lcu = (int)blockIdx.x * 4 + wave;
    const bool active = lcu < lcus;
    const int n = active ? lcu : lcus - 1; /* a wave past the last LCU computes the last one again and stores nothing */
    const int col = n % lcus_w, row = n / lcus_w, ox = col * 64, oy = row * 64;
    const bool complete = ox + 64 <= width && oy + 64 <= height;
    const bool logo = detect_logo_lcu(ox, oy, width, height, svt_amd_logo_cols(J.cls), svt_amd_logo_rows(J.cls));
    const int slice = J.slice, layer = J.layer;

    /* EbHevcGetMv of the LCU (lane 0) and of its left, top, right, bottom neighbour (lanes 1..4): 0 / 0 outside the bounds of :261-294.  An incomplete
     * neighbour inside them is read: its record exists */
    const int at = b == 1 ? n - 1 : b == 2 ? n - lcus_w : b == 3 ? n + 1 : b == 4 ? n + lcus_w : n;
    const bool there = b == 1 ? col > 0 : b == 2 ? row > 0 : b == 3 ? ox + 128 <= width : b == 4 ? oy + 128 <= height : b == 0;
    uint32_t word = 0;
    if (J.me && there)
        __builtin_memcpy(&word, &J.me[at], 4); /* pu[0].x_mv_l0, .y_mv_l0 */
    const int x = (int16_t)(word & 0xFFFFu), y = (int16_t)(word >> 16);
    const int cx = __shfl(x, 0), cy = __shfl(y, 0);

    /* Part1 / Part2 */
    const SvtAmdPaLcuStats &S = J.stats[n];
    const unsigned long long var0 = S.variance[1], var1 = S.variance[2], var2 = S.variance[3], var3 = S.variance[4];
    const unsigned long long average = (var0 + var1 + var2 + var3) >> 2;
    const int32_t d0 = (int32_t)(var0 - average), d1 = (int32_t)(var1 - average), d2 = (int32_t)(var2 - average), d3 = (int32_t)(var3 - average);
    /* the int sum of the four int products, converted to EB_U64 (:527-530); exact for 8-bit pictures, whose variances stay below 16,384 */
    const int32_t squares = (int32_t)((uint32_t)(d0 * d0) + (uint32_t)(d1 * d1) + (uint32_t)(d2 * d2) + (uint32_t)(d3 * d3));
    const unsigned long long var_of_var = (unsigned long long)(long long)squares >> 2;
    const bool low_motion = layer == 0 || (abs(cx) < 16 && abs(cy) < 16);
    const bool check1 = logo && complete && var_of_var > 50000 && low_motion, pm_check1 = logo && complete && var_of_var > 1000;
    bool low_dist = false;
    if (J.look_ahead && logo && complete && slice == 2) /* wave-uniform; the host made sure that the records are there */
        low_dist = J.me[n].pu[0].distortion[0] < 64u * 64u * (J.cls < 2 ? 5u : 2u);

    /* EbHevcDetectGlobalMotion: lanes 1..4 hold a candidate */
    const int th = 2 << (J.hier - layer); /* GLOBAL_MOTION_THRESHOLD[hierarchicalLevels][temporalLayerIndex] */
    const bool checked = complete && slice != 0, cand = checked && b >= 1 && b < 5;
    const bool pan_amp = cx * x > 0 && abs(cx) >= th && abs(x) >= th && abs(cx - x) < 64;
    const bool tilt_amp = cy * y > 0 && abs(cy) >= th && abs(y) >= th && abs(cy - y) < 64;
    const bool pan = __ballot(cand && cy < 64 && y < 64 && pan_amp) != 0, tilt = __ballot(cand && cx < 64 && x < 64 && tilt_amp) != 0;
    const bool pan_high = __ballot(cand && pan_amp) != 0, tilt_high = __ballot(cand && tilt_amp) != 0;
    const uint32_t votes = (uint32_t)pan | (uint32_t)tilt << 1 | (uint32_t)pan_high << 2 | (uint32_t)tilt_high << 3;

    if (b == 0) {
        s_part[wave] = active ? (uint32_t)checked | (uint32_t)pan << IRC_P_SHIFT | (uint32_t)tilt << 2 * IRC_P_SHIFT | (uint32_t)pan_high << 3 * IRC_P_SHIFT |
                                    (uint32_t)tilt_high << 4 * IRC_P_SHIFT
                              : 0u;
        if (active) {
            SvtAmdIrcChecks c;
            c.check1 = check1, c.pm_check1 = pm_check1, c.check2 = J.look_ahead != 0, c.low_dist_logo = low_dist;
            J.checks[n] = c;
            J.votes[n] = (uint8_t)votes;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0)
        J.part[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3]; /* a field is 4 at most */
}

/* grid (pictures), a workgroup of 256 threads per picture */
__global__ __launch_bounds__(IRC_MOTION_THREADS) void k_irc_motion(const IrcJobDev *__restrict__ jobs, int groups)
{
    __shared__ uint32_t red[IRC_MOTION_THREADS / 64];
    const IrcJobDev &J = jobs[blockIdx.x];
    uint32_t checked = 0, pan = 0, tilt = 0, pan_high = 0, tilt_high = 0;
    for (int g = threadIdx.x; g < groups; g += IRC_MOTION_THREADS) {
        const uint32_t p = J.part[g];
        checked += p & 15u, pan += p >> IRC_P_SHIFT & 15u, tilt += p >> 2 * IRC_P_SHIFT & 15u, pan_high += p >> 3 * IRC_P_SHIFT & 15u, tilt_high += p >> 4 * IRC_P_SHIFT & 15u;
    }
    checked = irc_block_sum<IRC_MOTION_THREADS / 64>(checked, red), pan = irc_block_sum<IRC_MOTION_THREADS / 64>(pan, red);
    tilt = irc_block_sum<IRC_MOTION_THREADS / 64>(tilt, red), pan_high = irc_block_sum<IRC_MOTION_THREADS / 64>(pan_high, red);
    tilt_high = irc_block_sum<IRC_MOTION_THREADS / 64>(tilt_high, red);
    if (threadIdx.x == 0) {
        SvtAmdIrcMotion m; /* every byte of the record is stored */
        m.total_checked_lcus = checked, m.total_pan_lcus = pan, m.total_tilt_lcus = tilt, m.total_pan_high_amp_lcus = pan_high, m.total_tilt_high_amp_lcus = tilt_high;
        m.is_pan_raw = checked && pan * 100u / checked > 75u, m.is_tilt_raw = checked && tilt * 100u / checked > 75u; /* PAN_LCU_PERCENTAGE */
        m.pad[0] = 0, m.pad[1] = 0;
        *J.motion = m;
    }
}

/* grid (LCUs / 4, pictures): one wave per LCU */
__global__ __launch_bounds__(256) void k_irc_counts(const IrcJobDev *__restrict__ jobs, int lcus)
{
    const IrcJobDev &J = jobs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int lcu = (int)blockIdx.x * 4 + wave;
    const bool active = lcu < lcus;
    const int n = active ? lcu : lcus - 1; /* a wave past the last LCU computes the last one again and stores nothing */

    /* EbHevcStationaryEdgeCountLcu over the entries that count: lane b < 32 = 16x16 unit b & 15 of the plain (b < 16) or the PM flavour.  check1 and pm_check1
     * hold on complete potentialLogoLcu LCUs only, so they stand for the whole condition of :407 / :420 */
    const SvtAmdIrcChecks own = J.checks[n];
    const bool pm = (b & 16) != 0, eligible = b < 32 && (pm ? own.pm_check1 : own.check1) && own.check2;
    uint32_t count = 0;
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (e < J.edge_count) { /* wave-uniform */
            const SvtAmdIrcChecks c = J.edge_checks[e][n];
            const uint32_t edge = J.edge_detect[e][n].edge_cu;
            count += (pm ? c.pm_check1 : c.check1) ? edge >> (b & 15) & 1u : 0u;
        }
    count = eligible ? count : 0u; /* the memset's 0 elsewhere */
    /* StationaryEdgeOverUpdateOverTimeLcu, first loop: slideWindowTh is unsigned - 0xFFFFFFFF below four pictures */
    const uint32_t slide_th = (uint32_t)J.frames / 4u - 1u;
    const unsigned long long over = __ballot(eligible && count > slide_th);
    const bool edge_flag = __popcll(over & 0xFFFFull) >= 4, pm_edge_flag = __popcll(over >> 16 & 0xFFFFull) >= 4;

    /* UpdateHomogeneityOverTime: lane 32 + e = entry e of its window.  The square is the int product of two promoted EB_U16 */
    const int e = b - 32;
    uint32_t var = 0;
    if (e >= 0 && e < J.hom_count)
        var = J.hom_stats[e][n].variance[0];
    const unsigned long long sum = irc_wave_sum(var), sum_sqr = irc_wave_sum64((unsigned long long)(long long)(int32_t)(var * var));
    unsigned long long var_of_var = ~0ull; /* ResetHomogeneityStructures */
    bool homogeneous = false;
    if (J.look_ahead) {
        const unsigned long long divisor = (unsigned long long)J.frames - 1ull; /* noFramesToCheck - 1, not the entries walked (:707) */
        const unsigned long long mean_sqr = divisor ? sum_sqr / divisor : 0ull, mean = divisor ? sum / divisor : 0ull;
        var_of_var = mean_sqr - mean * mean;
        homogeneous = var_of_var <= 4096ull; /* VAR_BASED_DETAIL_PRESERVATION_SELECTOR_THRSLHD */
    }
    if (active) {
        SvtAmdIrcLcu &o = J.lcu[n]; /* every byte of the record is stored: bytes 0..31 a lane each, the rest lane 32 */
        if (b < 32)
            ((uint8_t *)&o)[b] = (uint8_t)count;
        if (b == 32) {
            o.var_of_var_over_time = var_of_var, o.homogeneous_over_time = homogeneous, o.motion_votes = J.votes[n];
#pragma unroll
            for (int i = 0; i < 6; i++)
                o.pad[i] = 0;
            J.flags[n] = (uint8_t)((edge_flag ? IRC_F_EDGE : 0) | (pm_edge_flag ? IRC_F_PM_EDGE : 0) | (homogeneous ? IRC_F_HOMOGENEOUS : 0));
        }
    }
}

/* one pass of StationaryEdgeOverUpdateOverTimeLcu's second half over both planes: PASS 0 = (a) :1197-1244, 1 = (b) :1258 / :1330, 2 = (c) :1288 / :1360.  Every
 * pass is a gather over the values in front of it: (b) and (c) write only LCUs whose flag is 0 and count a value they never write; (a) runs in place in raster
 * order in the reference, and an LCU is cleared there exactly when its flag is 1 and no neighbour's flag was 1 before the pass (tests/test_irc_cpu.py) */
template <int PASS> __device__ __forceinline__ uint32_t irc_pass(const uint8_t *src, int n, int lcus_w, int lcus_h)
{
    const int col = n % lcus_w, row = n / lcus_w;
    const int c0 = col > 0 ? col - 1 : col, c1 = col < lcus_w - 1 ? col + 1 : col, r0 = row > 0 ? row - 1 : row, r1 = row < lcus_h - 1 ? row + 1 : row;
    const uint32_t want = PASS == 2 ? 2u : 1u;
    uint32_t near = 0, near_pm = 0;
    for (int r = r0; r <= r1; r++)
        for (int c = c0; c <= c1; c++) {
            const uint32_t v = src[r * lcus_w + c];
            near += (v & 3u) == want, near_pm += (v >> 2 & 3u) == want;
        }
    const uint32_t v = src[n], gate = v & IRC_L_GATE;
    uint32_t f = v & 3u, pm = v >> 2 & 3u;
    if (PASS == 0) { /* the window holds the LCU itself */
        f = f == 1 && near == 1 ? 0u : f, pm = pm == 1 && near_pm == 1 ? 0u : pm;
    } else if (PASS == 1) {
        f = f == 0 && gate && near > 0 ? 2u : f, pm = pm == 0 && gate && near_pm > 0 ? 2u : pm;
    } else {
        f = f == 0 && gate && near > 3 ? 3u : f, pm = pm == 0 && gate && near_pm > 3 ? 3u : pm;
    }
    return f | pm << 2 | gate;
}

/* grid (pictures), a workgroup of 1024 threads per picture; dynamic LDS: two rows of a byte per LCU (each rounded up to 16 bytes) */
__global__ __launch_bounds__(IRC_FINISH_THREADS) void k_irc_finish(const IrcJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t irc_lds[];
    __shared__ uint32_t red[IRC_FINISH_THREADS / 64];
    const IrcJobDev &J = jobs[blockIdx.x];
    const int t = threadIdx.x, lcus = lcus_w * lcus_h, row_bytes = (lcus + 15) & ~15;
    uint8_t *first = irc_lds, *second = irc_lds + row_bytes;
    const int cols = svt_amd_logo_cols(J.cls), rows = svt_amd_logo_rows(J.cls);

    uint32_t homogeneous = 0;
    for (int n = t; n < lcus; n += IRC_FINISH_THREADS) {
        const int ox = n % lcus_w * 64, oy = n / lcus_w * 64;
        const bool complete = ox + 64 <= width && oy + 64 <= height;
        const uint32_t f = J.flags[n];
        const bool gate = detect_logo_lcu(ox, oy, width, height, cols, rows) && (J.checks[n].check2 || !complete);
        first[n] = (uint8_t)((f & IRC_F_EDGE ? 1u : 0u) | (f & IRC_F_PM_EDGE ? 4u : 0u) | (gate ? IRC_L_GATE : 0u));
        homogeneous += f & IRC_F_HOMOGENEOUS ? 1u : 0u;
    }
    __syncthreads();
    for (int n = t; n < lcus; n += IRC_FINISH_THREADS)
        second[n] = (uint8_t)irc_pass<0>(first, n, lcus_w, lcus_h);
    __syncthreads();
    for (int n = t; n < lcus; n += IRC_FINISH_THREADS)
        first[n] = (uint8_t)irc_pass<1>(second, n, lcus_w, lcus_h);
    __syncthreads();
    uint32_t hist0 = 0, hist1 = 0, hist2 = 0, hist3 = 0;
    for (int n = t; n < lcus; n += IRC_FINISH_THREADS) {
        const uint32_t v = irc_pass<2>(first, n, lcus_w, lcus_h), f = v & 3u;
        J.stationary[n] = (uint8_t)f, J.pm_stationary[n] = (uint8_t)(v >> 2 & 3u);
        hist0 += f == 0, hist1 += f == 1, hist2 += f == 2, hist3 += f == 3;
    }
    for (int n = lcus + t; n < ((lcus + 63) & ~63); n += IRC_FINISH_THREADS) /* the tail of the picture's bytes */
        J.stationary[n] = 0, J.pm_stationary[n] = 0;
    homogeneous = irc_block_sum<IRC_FINISH_THREADS / 64>(homogeneous, red);
    hist0 = irc_block_sum<IRC_FINISH_THREADS / 64>(hist0, red), hist1 = irc_block_sum<IRC_FINISH_THREADS / 64>(hist1, red);
    hist2 = irc_block_sum<IRC_FINISH_THREADS / 64>(hist2, red), hist3 = irc_block_sum<IRC_FINISH_THREADS / 64>(hist3, red);

    if (t == 0) {
        SvtAmdIrcPic p; /* every byte of the record is stored */
        if (J.look_ahead) { /* EbHevcUpdateGlobalMotionDetectionOverTime: the caller's list holds the non-I entries only */
            uint32_t pan_pictures = 0;
            for (int k = 0; k < J.pan_count; k++)
                pan_pictures += J.pan_motion[k]->is_pan_raw == 1;
            p.is_pan = J.slice != 0 && J.pan_count && pan_pictures * 100u / J.pan_count > 75u;
            p.is_tilt = 0; /* set to EB_FALSE (:488) and never set again */
        } else
            p.is_pan = J.motion->is_pan_raw, p.is_tilt = J.motion->is_tilt_raw;
        p.homogeneity_percentage = (uint8_t)(homogeneous * 100u / (uint32_t)lcus);
        p.pad0 = 0, p.homogeneous_lcu_count = (uint16_t)homogeneous;
        p.stationary_lcu_count[0] = (uint16_t)hist0, p.stationary_lcu_count[1] = (uint16_t)hist1, p.stationary_lcu_count[2] = (uint16_t)hist2;
        p.stationary_lcu_count[3] = (uint16_t)hist3;
        p.pad[0] = 0, p.pad[1] = 0;
        *J.pic = p;
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

extern "C" size_t svt_amd_initial_rc_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    const size_t lcus = (size_t)svt_amd_lcu_count(luma_width, luma_height);
    switch (which) {
    case SVT_AMD_IRC_CHECKS:
        return lcus * sizeof(SvtAmdIrcChecks);
    case SVT_AMD_IRC_MOTION:
        return sizeof(SvtAmdIrcMotion);
    case SVT_AMD_IRC_LCU:
        return lcus * sizeof(SvtAmdIrcLcu);
    case SVT_AMD_IRC_STATIONARY:
    case SVT_AMD_IRC_PM_STATIONARY:
        return (lcus + 63) & ~(size_t)63;
    case SVT_AMD_IRC_PICTURE:
        return sizeof(SvtAmdIrcPic);
    }
    return 0;
}

/* the rules of a picture that read its ME records: a vector above layer 0 (Part1) and in P / B pictures (EbHevcDetectGlobalMotion), a distortion in B pictures */
static bool irc_reads_me(const SvtAmdIrcJob &j) { return j.slice_type != 0 || j.temporal_layer_index > 0; }

extern "C" int svt_amd_initial_rc_batch_launch(SvtAmdContext *ctx, const SvtAmdIrcJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                               const SvtAmdIrcArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    SvtAmdBatchGeometry g;
    SVT_AMD_TRY(svt_amd_batch_geometry(__func__, ctx, luma_width, luma_height, SVT_AMD_IRC_MAX_LCUS, true, &g));
    const auto [w, h, wl, hl, lcus, groups, cap_lcus, cap_groups] = g;
    if (!out->checks || !out->motion || !out->lcu || !out->stationary_edge || !out->pm_stationary_edge || !out->picture)
        SVT_AMD_BAD("%s: job 0: there is no %s array", __func__, !out->checks ? "checks" : !out->motion ? "motion" : !out->lcu ? "lcu" :
                    !out->stationary_edge ? "stationary_edge" : !out->pm_stationary_edge ? "pm_stationary_edge" : "picture");
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdIrcJob &j = jobs[i];
        if (!j.stats)
            SVT_AMD_BAD("%s: job %d has no block statistics", __func__, i);
        if (j.slice_type > 2 || j.hierarchical_levels > 5 || j.temporal_layer_index > j.hierarchical_levels || j.resolution_class > 3)
            SVT_AMD_BAD("%s: job %d: slice type %d, temporal layer %d, hierarchical levels %d, resolution class %d", __func__, i, j.slice_type, j.temporal_layer_index,
                        j.hierarchical_levels, j.resolution_class);
        if (j.frames_to_check < 1 || j.frames_to_check > 17)
            SVT_AMD_BAD("%s: job %d: %d frames to check (1..17)", __func__, i, j.frames_to_check);
        if (j.edge_count > 4 || j.hom_count > 16 || j.pan_count > 8)
            SVT_AMD_BAD("%s: job %d: look-ahead lists of %d, %d and %d entries (at most 4, 16 and 8)", __func__, i, j.edge_count, j.hom_count, j.pan_count);
        if (!j.look_ahead && (j.edge_count || j.hom_count || j.pan_count || j.frames_to_check != 1))
            SVT_AMD_BAD("%s: job %d has no look-ahead, but lists of %d, %d and %d entries and %d frames to check", __func__, i, j.edge_count, j.hom_count, j.pan_count,
                        j.frames_to_check);
        for (int k = 0; k < j.edge_count; k++)
            if (!j.edge_checks[k] || !j.edge_detect[k])
                SVT_AMD_BAD("%s: job %d: %s[%d] of %d entries is NULL", __func__, i, j.edge_checks[k] ? "edge_detect" : "edge_checks", k, j.edge_count);
        for (int k = 0; k < j.hom_count; k++)
            if (!j.hom_stats[k])
                SVT_AMD_BAD("%s: job %d: hom_stats[%d] of %d entries is NULL", __func__, i, k, j.hom_count);
        for (int k = 0; k < j.pan_count; k++)
            if (!j.pan_motion[k])
                SVT_AMD_BAD("%s: job %d: pan_motion[%d] of %d entries is NULL", __func__, i, k, j.pan_count);
        if (irc_reads_me(j) && !j.me) /* the records resident in the slot */
            SVT_AMD_TRY(svt_amd_batch_slot_records(__func__, ctx, i, j.cur_slot, BATCH_REC_ME, w, h));
    }

    IrcJobDev *d_tab;
    uint8_t *d_scratch; /* per picture: a word per workgroup of k_irc_lcu, then a vote byte and a flag byte per LCU */
    const size_t lcu_bytes = (size_t)((cap_lcus + 3) & ~3), pic_scratch = (size_t)cap_groups * 4 + 2 * lcu_bytes;
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_IRC, sizeof(IrcJobDev), pic_scratch * SVT_AMD_MAX_BATCH, (void **)&d_tab, (void **)&d_scratch));
    static thread_local IrcJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    SvtAmdRecordsBinder bind;
    const size_t edge_bytes = (size_t)((lcus + 63) & ~63);
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdIrcJob &j = jobs[i];
        IrcJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        if (irc_reads_me(j)) {
            d.me = j.me;
            if (!j.me)
                SVT_AMD_TRY(svt_amd_batch_bind_records(ctx, &bind, j.cur_slot, SLOT_ME, (const void **)&d.me));
        }
        d.stats = j.stats;
        for (int k = 0; k < j.edge_count; k++)
            d.edge_checks[k] = j.edge_checks[k], d.edge_detect[k] = j.edge_detect[k];
        for (int k = 0; k < j.hom_count; k++)
            d.hom_stats[k] = j.hom_stats[k];
        for (int k = 0; k < j.pan_count; k++)
            d.pan_motion[k] = j.pan_motion[k];
        d.checks = out->checks + (size_t)i * lcus, d.motion = out->motion + i, d.lcu = out->lcu + (size_t)i * lcus;
        d.stationary = out->stationary_edge + (size_t)i * edge_bytes, d.pm_stationary = out->pm_stationary_edge + (size_t)i * edge_bytes;
        d.pic = out->picture + i;
        uint8_t *scratch = d_scratch + (size_t)i * pic_scratch;
        d.part = (uint32_t *)scratch, d.votes = scratch + (size_t)cap_groups * 4, d.flags = d.votes + lcu_bytes;
        d.edge_count = j.edge_count, d.hom_count = j.hom_count, d.pan_count = j.pan_count, d.slice = j.slice_type, d.layer = j.temporal_layer_index;
        d.hier = j.hierarchical_levels, d.cls = j.resolution_class, d.look_ahead = j.look_ahead != 0, d.frames = j.frames_to_check;
    }
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(IrcJobDev) * (size_t)num_jobs));
    /* the stages are ordered on the lane, and the scratch is stored into, never added to: a batch queued behind this one overwrites it only after this one's
     * kernels have read it, and there is nothing to zero */
    hipLaunchKernelGGL(k_irc_lcu, dim3((unsigned)groups, (unsigned)num_jobs), dim3(256), 0, st, (const IrcJobDev *)d_tab, w, h, wl, lcus);
    hipLaunchKernelGGL(k_irc_motion, dim3((unsigned)num_jobs), dim3(IRC_MOTION_THREADS), 0, st, (const IrcJobDev *)d_tab, groups);
    hipLaunchKernelGGL(k_irc_counts, dim3((unsigned)groups, (unsigned)num_jobs), dim3(256), 0, st, (const IrcJobDev *)d_tab, lcus);
    hipLaunchKernelGGL(k_irc_finish, dim3((unsigned)num_jobs), dim3(IRC_FINISH_THREADS), 2 * (size_t)((lcus + 15) & ~15), st, (const IrcJobDev *)d_tab, w, h, wl, hl);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
