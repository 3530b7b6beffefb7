/*
 * mdc_kernels.hip - ModeDecisionConfigurationKernel (Codec/EbModeDecisionConfigurationProcess.c:1905) with EarlyModeDecisionLcu
 * (Codec/EbModeDecisionConfiguration.c:1059) for P / B pictures in the batched, stream-ordered shape of sbo_kernels.hip (include/svt_hevc_amd.h "Batched
 * mode-decision configuration"): the picture is a grid dimension, the per-picture pointers come from a descriptor table in device memory, nothing
 * is copied to the host.  Integer logic on records; no plane is read.  Restated as tests/mdc_numpy.py spells it out: every EB_U32 expression wraps at 32 bits.
 *   k_mdc_lcu       grid (LCUs / 4, pictures), a wave per LCU.  AuraDetection (:791-939), the deciding clause of IsAvcPartitioningMode (:1232), the P / B arm of
 *                   DeriveLcuScore (:1596; a partial LCU: a lane per 8x8 unit, wave sum).  It STORES the score and the AVC flag into context-owned scratch and
 *                   the aura status into the LCU's record; lane 0 of workgroup 0 writes the picture signals (:1949-1975, :112, :175).
 *   k_mdc_budget    grid (pictures), a workgroup of 1024 threads per picture, PICT_LCU_SWITCH pictures only.  Minimum / maximum, PerformOutlierRemoval (:1736),
 *                   ConfigureAdp, SetTargetBudgetOq (:1079), DeriveDefaultSegments (:942), ComputeRefinementCost, then the passes of DeriveOptimalBudgetPerLcu /
 *                   SetLcuBudget: the scores lie in LDS, a pass is a map over them and one workgroup-wide sum; every thread holds the same thresholds and
 *                   shooting state and updates them from the same sum, so the exit test is uniform.  DeriveSearchMethod (:1360-1392).
 *   k_mdc_leaves    grid (LCUs / 4, pictures), a wave per LCU: the leaf list.  A lane per coded unit (lanes 0..63 = MD-scan units 0..63, lanes 0..20 again =
 *                   units 64..84); the valid / root / selected / stop sets of the 85 units are wave ballots - two 64-bit scalars each, no array, no scratch;
 *                   the list is a compaction: a unit's place is the population count of the emitted set below it.
 * Bound: latency - 184 B written and a few hundred bytes read per LCU, 21 ME units of the open-loop LCUs.
 */
#include "pa_batch.h"
#include <string.h>

struct MdcJobDev {
    const SvtAmdMeLcuResult *me;
    const SvtAmdPaLcuStats *stats;
    const SvtAmdPaLcuDetect *detect;
    const SvtAmdSboLcu *sbo_lcu;
    const SvtAmdSboPic *sbo_pic;
    const SvtAmdPaPicDetect *pic_detect;
    const SvtAmdNoisePic *noise_pic;
    const uint8_t *stationary; /* or null */
    SvtAmdMdcLcu *lcu;
    SvtAmdMdcPic *pic;
    uint32_t *score;           /* [lcus]: DeriveLcuScore, context-owned scratch */
    uint8_t *avc;              /* [lcus]: IsAvcPartitioningMode, context-owned scratch */
    uint32_t lambda, split_bits[2];
    uint8_t slice, layer, hier, is_ref, depth_mode, enc_mode, cls, qp, pan, tilt, ndth, homog, fr30, cu8, avg_int, ref_int[2], ref_skip[2], pad;
};
static_assert(sizeof(MdcJobDev) == 128, "MdcJobDev layout");
static_assert(sizeof(SvtAmdMdcJob) == 104 && sizeof(SvtAmdMdcLcu) == 184 && sizeof(SvtAmdMdcPic) == 48, "mode-decision configuration records");
static_assert(offsetof(SvtAmdMdcLcu, lcu_md_mode) == 171 && offsetof(SvtAmdMdcLcu, lcu_score) == 176 && offsetof(SvtAmdMdcLcu, lcu_cost) == 180, "SvtAmdMdcLcu layout");
static_assert(offsetof(SvtAmdMdcPic, adp_depth_sensitive_picture_class) == 8 && offsetof(SvtAmdMdcPic, score_th) == 28, "SvtAmdMdcPic layout");

/* EB_PICTURE_DEPTH_MODE - 1 / EB_LCU_DEPTH_MODE (Codec/EbDefinitions.h:1262-1280) */
enum { MDC_PICT_LCU_SWITCH = 0, MDC_PICT_FULL85 = 1, MDC_PICT_FULL84 = 2 };
enum { MDC_FULL85 = 1, MDC_FULL84, MDC_BDP, MDC_LIGHT_BDP, MDC_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_AVC, MDC_LIGHT_AVC, MDC_PRED_OPEN_LOOP, MDC_PRED_OPEN_LOOP_1_NFL };
#define MDC_INVALID_AURA 128
#define MDC_BUDGET_THREADS 1024
#define MDC_BUDGET_WAVES (MDC_BUDGET_THREADS / 64)

/* a table of six rows whose entries past the diagonal are 0, as the reference's initialisers leave them: selects, not loads */
__device__ __forceinline__ int mdc_row6(int i, int a, int b, int c, int d, int e, int f) { return i == 0 ? a : i == 1 ? b : i == 2 ? c : i == 3 ? d : i == 4 ? e : f; }
__device__ __forceinline__ int mdc_global_motion_th(int hier, int layer) { return layer <= hier ? 2 << (hier - layer) : 0; } /* GlobalMotionThreshold */
__device__ __forceinline__ int mdc_luminosity_th(int hier, int layer) /* AdpLuminosityChangeThArray */
{
    const int v = mdc_row6(hier, 0x2, 0x22, 0x223, 0x2233, 0x22334, 0x223344); /* a nibble per layer, the last layer lowest */
    return layer <= hier ? v >> 4 * (hier - layer) & 15 : 0;
}
__device__ __forceinline__ int mdc_intra_area_th0(int hier) { return mdc_row6(hier, 20, 30, 40, 50, 50, 50); } /* INTRA_AREA_TH_CLASS_1[hier][0] */
__device__ __forceinline__ int mdc_qp_offset_layer(int hier, int layer) /* MOD_QP_OFFSET_LAYER_ARRAY */
{
    const int v = mdc_row6(hier, 0x1, 0x65, 0x543, 0x5531, 0x65531, 0x765531); /* a nibble per layer, layer 0 lowest */
    return layer <= hier ? v >> 4 * layer & 15 : 0;
}
/* costDepthMode (ConfigureAdp :1288) by EB_LCU_DEPTH_MODE */
__device__ __forceinline__ uint32_t mdc_mode_cost(int m)
{
    return m <= MDC_FULL84 ? 155u : m == MDC_BDP ? 129u : m == MDC_LIGHT_BDP ? 123u : m == MDC_OPEN_LOOP ? 110u : m == MDC_LIGHT_OPEN_LOOP ? 106u : m == MDC_AVC ? 138u :
           m == MDC_LIGHT_AVC ? 122u : m == MDC_PRED_OPEN_LOOP ? 100u : 97u;
}

/* the picture signals both per-LCU stages need: sceneCaracteristicId (:1949-1967) and highIntraSlection (:212-240) */
__device__ __forceinline__ void mdc_scene(const MdcJobDev &J, int &scene, int &high_intra)
{
    const int grass = J.sbo_pic->grass_percentage, noise = J.noise_pic->pic_noise_class, th = J.ndth == 0 ? 1 : 3;
    scene = 0;
    if (!J.pan && !J.tilt && grass > 0 && grass <= 35 && noise >= th && J.homog < 50)
        scene = 1;
    if (J.pan && !J.tilt && grass > 35 && grass <= 70 && noise >= th && J.homog < 50)
        scene = 2;
    high_intra = 0;
    if (J.slice == 2)
        high_intra = J.layer == 0 ? (int)J.sbo_pic->intra_coded_block_probability > mdc_intra_area_th0(J.hier) : (J.ref_skip[0] || J.ref_skip[1]);
}

__device__ __forceinline__ uint32_t mdc_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += (uint32_t)__shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t mdc_wave_min(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t mdc_wave_max(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

/* grid (LCUs / 4, pictures): one wave per LCU */
__global__ __launch_bounds__(256) void k_mdc_lcu(const MdcJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    const MdcJobDev &J = jobs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int lcus = lcus_w * lcus_h, lcu = (int)blockIdx.x * 4 + wave;
    const bool active = lcu < lcus;
    const int n = active ? lcu : lcus - 1; /* a wave past the last LCU computes the last one again and stores nothing */
    const int col = n % lcus_w, row = n / lcus_w, ox = col * 64, oy = row * 64;
    const bool complete = ox + 64 <= width && oy + 64 <= height;
    const bool edge = ox < 64 || oy < 64 || ox > width - 64 || oy > height - 64; /* isEdgeLcu (Codec/EbSequenceControlSet.c:210) */
    const int slice = J.slice, layer = J.layer, cls = J.cls;
    int scene, high_intra;
    mdc_scene(J, scene, high_intra);
    const SvtAmdSboPic &SP = *J.sbo_pic;
    const SvtAmdMeCuResult &U = J.me[n].pu[0];

    /* AuraDetection / AuraDetection64x64: the four neighbours exist for every LCU that is no edge LCU */
    int aura = MDC_INVALID_AURA;
    if (slice == 2 && col > 0 && col < lcus_w - 1 && row < lcus_h - 1) {
        aura = 0;
        if (!edge) {
            int mv0x = 0, mv0y = 0, mv1x = 0, mv1y = 0;
            const int total = min((int)U.total_me_candidate_index, 3);
            for (int k = 0; k < total; k++) {
                if (U.direction[k] == 0)
                    mv0x = U.x_mv_l0, mv0y = U.y_mv_l0;
                if (U.direction[k] == 1)
                    mv1x = U.x_mv_l1, mv1y = U.y_mv_l1;
            }
            uint32_t th0 = J.is_ref || cls == 3 ? 15u : 14u; /* the second threshold (23) decides nothing: AURA_STATUS_1 is the only status set */
            if (J.qp > 38)
                th0 <<= 2;
            const int gmt = mdc_global_motion_th(J.hier, layer);
            const uint32_t cur = U.distortion[0];
            if (cur > 64 * 64 && (abs(mv0x) > gmt || abs(mv0y) > gmt || abs(mv1x) > gmt || abs(mv1y) > gmt)) {
                const uint32_t top = J.me[n - lcus_w].pu[0].distortion[0], top_l = J.me[n - lcus_w - 1].pu[0].distortion[0], left = J.me[n - 1].pu[0].distortion[0];
                const uint32_t top_r = col < lcus_w - 2 ? J.me[n - lcus_w + 1].pu[0].distortion[0] : cur;
                const uint32_t right = top_r; /* :888: rightDist is assigned from topRDist; the right neighbour's distortion is never used */
                const uint32_t local = min(min(min(top_l, min(top_r, top)), left), right);
                if (10u * cur > th0 * local)
                    aura = 1;
            }
        }
    }

    uint32_t score = 0;
    int avc = 0;
    if (J.depth_mode == MDC_PICT_LCU_SWITCH) {
        /* IsAvcPartitioningMode: the first clause that holds */
        if (cls > 1) {
            if (SP.high_dark_low_light_area_density && layer > 0 && J.detect[n].sharp_edge && !J.sbo_lcu[n].similar_colocated_all_layers)
                avc = 1;
            else if (scene == 0 && SP.grass_percentage > 60 && aura == 1 && high_intra == 0 && complete)
                avc = 2;
            else if (J.pic_detect->logo_pic && J.detect[n].edge_block_num)
                avc = 3;
            else if (J.stationary && J.stationary[n] > 0)
                avc = 4;
            else if (J.sbo_lcu[n].complex_lcu == 2)
                avc = 5;
        }
        /* DeriveLcuScore, P / B */
        const uint32_t cmin = SP.inter_complexity_min[0], cmax = SP.inter_complexity_max[0], nm_avg = SP.non_moving_index_average;
        if (!complete) { /* the wrapping mean of the valid 8x8 units' distortions: lane b = 8x8 unit b (raster) */
            const bool v8 = ox + (b & 7) * 8 + 8 <= width && oy + (b >> 3) * 8 + 8 <= height;
            const uint32_t total = mdc_wave_sum(v8 ? J.me[n].pu[21 + b].distortion[0] : 0u), count = (uint32_t)__popcll(__ballot(v8));
            if (count) {
                const uint32_t v = total / count * 64u;
                score = v < cmin ? cmin : v > cmax ? cmax : v;
            }
        } else {
            uint32_t s = U.distortion[0];
            const uint32_t nmi = J.sbo_lcu[n].non_moving_index;
            if (J.sbo_lcu[n].failing_motion)
                s = cmax;
            else if (edge && nmi != 0xFF && nm_avg != 0xFF && nmi >= 10 && (nmi >= nm_avg || nm_avg > 25) && cls == 3)
                s = s + (cmax - s) * 75u / 100u;
            else {
                if (nmi == 30 && J.stats[n].variance[0] > 100 && J.fr30)
                    s = s - (s - cmin) * 50u / 100u;
                const bool dark_lcu = J.stats[n].y_mean[0] < 25;
                if (cls != 3 || SP.black_area_percentage > 25)
                    s = dark_lcu ? s - (s - cmin) * 50u / 100u : s + (cmax - s) * 50u / 100u;
            }
            score = s;
        }
    }
    if (active && b == 0) {
        J.score[n] = score, J.avc[n] = (uint8_t)avc;
        SvtAmdMdcLcu &o = J.lcu[n]; /* k_mdc_budget overwrites mode, score and cost of a PICT_LCU_SWITCH picture; k_mdc_leaves writes bytes 0..175 */
        o.lcu_md_mode = 0, o.aura_status = (uint8_t)aura, o.avc_partitioning = avc != 0, o.lcu_score = 0;
        o.lcu_cost = 0, o.pad[0] = 0, o.pad[1] = 0, o.pad[2] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { /* the picture signals: the first eight bytes of the record */
        SvtAmdMdcPic &p = *J.pic;
        const int grass = SP.grass_percentage, noise = J.noise_pic->pic_noise_class, th = J.ndth == 0 ? 1 : 3;
        p.scene_characteristic_id = (uint8_t)scene;
        p.adjust_min_qp = !J.pan && !J.tilt && grass > 2 && grass <= 35 && J.homog < 70 && SP.zz_cost_average > 15 && noise >= th;
        p.high_intra_selection = (uint8_t)high_intra;
        const int offset = noise >= 7 ? 10 : noise >= 5 ? 8 : max(-12, min(12, mdc_qp_offset_layer(J.hier, layer) - 3));
        p.slice_cb_qp_offset = (int8_t)offset, p.slice_cr_qp_offset = (int8_t)offset;
        p.tc_offset = 0, p.beta_offset = 0, p.average_qp = J.qp;
    }
}

/* the sum over the workgroup's threads; every thread gets it.  red: MDC_BUDGET_WAVES words of LDS nobody touches until the next call's first barrier */
__device__ __forceinline__ uint32_t mdc_block_sum(uint32_t v, uint32_t *red)
{
    v = mdc_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < MDC_BUDGET_WAVES; i++)
        sum += red[i];
    return sum;
}

/* SetTargetBudgetOq (:1079) */
__device__ __forceinline__ uint32_t mdc_target_budget(uint32_t n, const MdcJobDev &J, int sens)
{
    const int enc = J.enc_mode, cls = J.cls, layer = J.layer;
    const bool ref = J.is_ref, pan_tilt = J.pan || J.tilt;
    const uint32_t adp = layer == 0 ? (sens == 2 ? n * 127u : sens == 1 ? n * 125u : n * 121u) : ref ? (sens == 2 ? n * 110u : n * 100u) : n * 100u;
    const uint32_t plain = layer == 0 ? n * 129u : ref ? n * 110u : n * 109u;
    if (enc <= 5) {
        if (cls <= 1)
            return layer == 0 ? n * 155u : ref ? (pan_tilt ? n * 152u : n * 150u) : (pan_tilt ? n * 152u : n * 145u);
        if (cls <= 2)
            return layer == 0 ? n * 155u : ref ? n * 138u : n * 134u;
        if (enc <= 3)
            return plain;
        return layer == 0 ? n * 155u : ref ? n * 125u : n * 121u;
    }
    if (enc <= 7)
        return plain;
    if (enc <= 8)
        return cls == 3 ? adp : plain;
    return adp;
}

/* the tests of one pass of SetLcuBudget (:1425-1445) for interval k < 6: (scoreToMin <= maxToMinScore * scoreTh[k] / 100 && scoreTh[k] != 0) || numberOfSegments ==
 * k + 1 || scoreTh[k + 1] == 100.  The product is 32 bits wide with the EB_S8 threshold converted to unsigned: -1 multiplies as 0xFFFFFFFF (:1431) */
__device__ __forceinline__ void mdc_pass_limits(uint32_t span, const int (&th)[7], int nseg, uint32_t (&limit)[6], bool (&ok)[6])
{
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const bool take = nseg == k + 1 || th[k + 1] == 100;
        limit[k] = take ? ~0u : span * (uint32_t)th[k] / 100u;
        ok[k] = take || th[k] != 0;
    }
}
/* the cost SetLcuBudget gives one LCU: avc = IsAvcPartitioningMode, to_min = its clamped score - lcuMinScore */
__device__ __forceinline__ uint32_t mdc_lcu_cost(bool avc, uint32_t to_min, int mode, int layer, const uint32_t (&interval)[7], const uint32_t (&limit)[6], const bool (&ok)[6])
{
    if (mode == 2 && avc)
        return 138;
    if (mode == 1 && avc)
        return 122;
    uint32_t cost = interval[6];
#pragma unroll
    for (int k = 5; k >= 0; k--) /* the first interval whose test holds */
        if (ok[k] && to_min <= limit[k])
            cost = interval[k];
    if (avc) {
        if (cost > 138)
            cost = 138;
        else if (cost > 122 && layer > 0)
            cost = 122;
    }
    return cost;
}

/* grid (pictures), a workgroup of 1024 threads per picture; dynamic LDS: the scores [lcus], then one bit per LCU (AVC), a word per wave of the load loop */
__global__ __launch_bounds__(MDC_BUDGET_THREADS) void k_mdc_budget(const MdcJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t mdc_lds[];
    __shared__ uint32_t red[MDC_BUDGET_WAVES], pass_red[2][MDC_BUDGET_WAVES];
    const MdcJobDev &J = jobs[blockIdx.x];
    const int t = threadIdx.x, lcus = lcus_w * lcus_h;
    const uint32_t n_lcus = (uint32_t)lcus;
    SvtAmdMdcPic &P = *J.pic;
    if (J.depth_mode != MDC_PICT_LCU_SWITCH) { /* workgroup-uniform: no budget is written (the fields stay 0) */
        if (t < 10)
            ((uint32_t *)&P)[2 + t] = 0;
        return;
    }
    uint32_t *s_score = mdc_lds;
    unsigned long long *s_avc = (unsigned long long *)(mdc_lds + ((lcus + 1) & ~1));
    const int rounds = (lcus + MDC_BUDGET_THREADS - 1) / MDC_BUDGET_THREADS;

    /* the scores and flags into LDS; minimum and maximum over every LCU, the count of AVC LCUs */
    uint32_t lo = ~0u, hi = 0, avc_n = 0;
    for (int r = 0; r < rounds; r++) { /* every wave runs every round: the ballot is of whole waves */
        const int n = r * MDC_BUDGET_THREADS + t;
        const bool in = n < lcus;
        const uint32_t s = in ? J.score[n] : 0u;
        const bool a = in && J.avc[n] != 0;
        if (in)
            s_score[n] = s, lo = min(lo, s), hi = max(hi, s);
        const unsigned long long m = __ballot(a);
        if ((t & 63) == 0 && (n & ~63) < lcus)
            s_avc[n >> 6] = m;
        avc_n += a;
    }
    lo = mdc_wave_min(lo), hi = mdc_wave_max(hi);
    __syncthreads();
    if ((t & 63) == 0)
        pass_red[0][t >> 6] = lo, pass_red[1][t >> 6] = hi;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MDC_BUDGET_WAVES; i++)
        lo = min(lo, pass_red[0][i]), hi = max(hi, pass_red[1][i]);
    avc_n = mdc_block_sum(avc_n, red);

    /* PerformOutlierRemoval: ten bins over the complete LCUs; (score + min) as written */
    const uint32_t sub = (hi - lo) / 10u;
    uint32_t hist[10], processed = 0;
#pragma unroll
    for (int k = 0; k < 10; k++)
        hist[k] = 0;
    for (int n = t; n < lcus; n += MDC_BUDGET_THREADS) {
        const int col = n % lcus_w, row = n / lcus_w;
        if (!(col * 64 + 64 <= width && row * 64 + 64 <= height))
            continue;
        processed++;
        const uint32_t v = s_score[n] + lo;
        bool placed = false;
#pragma unroll
        for (int k = 0; k < 10; k++) {
            const bool here = !placed && v < (uint32_t)(k + 1) * sub + lo;
            hist[k] += here, placed |= here;
        }
    }
    processed = mdc_block_sum(processed, red);
#pragma unroll
    for (int k = 0; k < 10; k++) {
        hist[k] = mdc_block_sum(hist[k], red);
        if (processed && hist[k] * 100u / processed < 2u)
            hist[k] = 0;
    }
    {
        uint32_t new_lo = lo, new_hi = hi;
        bool found = false;
#pragma unroll
        for (int k = 0; k < 10; k++)
            if (!found && hist[k])
                new_lo = lo + (uint32_t)k * sub, found = true;
        found = false;
#pragma unroll
        for (int k = 9; k >= 0; k--)
            if (!found && hist[k])
                new_hi = hi - (uint32_t)(9 - k) * sub, found = true;
        lo = new_lo, hi = new_hi;
    }

    /* ConfigureAdp (:1288) */
    const int layer = J.layer, noise = J.noise_pic->pic_noise_class;
    const bool ref = J.is_ref;
    bool lum = false;
    if (ref) {
        const int th = mdc_luminosity_th(J.hier, layer);
        lum = abs((int)J.avg_int - (int)J.ref_int[0]) >= th || (J.slice == 2 && abs((int)J.avg_int - (int)J.ref_int[1]) >= th);
    }
    const uint32_t nm_avg = J.sbo_pic->non_moving_index_average;
    int sens = 0;
    if (nm_avg != 0xFF && nm_avg < 30) {
        if (noise > 3 || J.sbo_pic->high_dark_low_light_area_density || lum)
            sens = 2;
        else if (nm_avg >= 15 && noise == 3)
            sens = 1;
    }
    const uint32_t budget = mdc_target_budget(n_lcus, J, sens);
    /* DeriveDefaultSegments (:942): the interval modes, a nibble each, the first lowest */
    int nseg;
    uint32_t modes;
#define MDC_MODES(a, b, c, d, e, f) ((uint32_t)(a) | (uint32_t)(b) << 4 | (uint32_t)(c) << 8 | (uint32_t)(d) << 12 | (uint32_t)(e) << 16 | (uint32_t)(f) << 20)
    if (layer == 0) {
        if (sens && budget >= n_lcus * 123u) {
            nseg = 2, modes = budget > n_lcus * 129u ? MDC_MODES(MDC_BDP, MDC_FULL84, 0, 0, 0, 0) : MDC_MODES(MDC_LIGHT_BDP, MDC_BDP, 0, 0, 0, 0);
        } else if (budget > n_lcus * 129u)
            nseg = 2, modes = MDC_MODES(MDC_BDP, MDC_FULL84, 0, 0, 0, 0);
        else if (budget > n_lcus * 110u)
            nseg = 4, modes = MDC_MODES(MDC_PRED_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_LIGHT_BDP, MDC_BDP, 0, 0);
        else
            nseg = 5, modes = MDC_MODES(MDC_PRED_OPEN_LOOP_1_NFL, MDC_PRED_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_LIGHT_BDP, MDC_BDP, 0);
    } else if (budget > n_lcus * 120u)
        nseg = 6, modes = MDC_MODES(MDC_PRED_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_OPEN_LOOP, MDC_LIGHT_BDP, MDC_BDP, MDC_FULL85);
    else if (budget > n_lcus * 115u)
        nseg = 5, modes = MDC_MODES(MDC_PRED_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_OPEN_LOOP, MDC_LIGHT_BDP, MDC_BDP, 0);
    else if (budget > n_lcus * 110u)
        nseg = 4, modes = MDC_MODES(MDC_PRED_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_OPEN_LOOP, MDC_LIGHT_BDP, 0, 0);
    else
        nseg = 4, modes = MDC_MODES(MDC_PRED_OPEN_LOOP_1_NFL, MDC_PRED_OPEN_LOOP, MDC_LIGHT_OPEN_LOOP, MDC_OPEN_LOOP, 0, 0);
#undef MDC_MODES
    int th[7];           /* scoreTh: EB_S8 values */
    uint32_t interval[7]; /* intervalCost */
#pragma unroll
    for (int k = 0; k < 7; k++) {
        th[k] = k < nseg - 1 ? (k + 1) * 100 / nseg : -1;
        interval[k] = k < nseg ? mdc_mode_cost((int)(modes >> 4 * k & 15u)) : 0u;
    }
    /* ComputeRefinementCost */
    const uint32_t avc_cost = avc_n * 138u + (n_lcus - avc_n) * interval[0], light_cost = avc_n * 122u + (n_lcus - avc_n) * interval[0];
    int mode;
    if (avc_cost <= budget && (budget > 123u * n_lcus || layer == 0 || (J.cls < 3 && ref)))
        mode = 2;
    else if (light_cost <= budget && layer > 0)
        mode = 1;
    else
        mode = 0;

    /* DeriveOptimalBudgetPerLcu / SetLcuBudget.  The clamp of the scores (:1420) gives the same values in every pass: done once.  It sits in the arm of the LCUs
     * that are budgeted by score: an AVC LCU of refinement mode 1 or 2 keeps the score DeriveLcuScore gave it */
    __syncthreads();
    for (int n = t; n < lcus; n += MDC_BUDGET_THREADS) {
        const uint32_t s = s_score[n];
        if (!(mode != 0 && (s_avc[n >> 6] >> (n & 63) & 1ull)))
            s_score[n] = s < lo ? lo : s > hi ? hi : s;
    }
    __syncthreads();
    const uint32_t span = hi - lo;
    uint32_t predicted = ~0u, deviation = 1000;
    int initial = 2, final_ = 2, iteration = 0; /* TBD_SHOOTING */
    uint32_t limit[6]; /* of the pass that ran last: the store pass below gives every LCU the cost that pass gave it */
    bool ok[6];
    while (deviation != 0 && initial == final_ && iteration <= 100) { /* every thread holds the same state: uniform */
        initial = predicted < budget ? 0 : 1; /* UNDER_SHOOTING / OVER_SHOOTING */
        mdc_pass_limits(span, th, nseg, limit, ok);
        uint32_t sum = 0;
        for (int n = t; n < lcus; n += MDC_BUDGET_THREADS)
            sum += mdc_lcu_cost(s_avc[n >> 6] >> (n & 63) & 1ull, s_score[n] - lo, mode, layer, interval, limit, ok);
        sum = mdc_wave_sum(sum);
        uint32_t *pr = pass_red[iteration & 1]; /* two rows in turn: one barrier a pass */
        if ((t & 63) == 0)
            pr[t >> 6] = sum;
        __syncthreads();
        predicted = 0;
#pragma unroll
        for (int i = 0; i < MDC_BUDGET_WAVES; i++)
            predicted += pr[i];
        /* ABS((EB_S32)(predictedCost - budget)) * 1000 (:1522): the signed product as written - below 2^31 for the pictures the launcher admits */
        deviation = (uint32_t)(abs((int32_t)(predicted - budget)) * 1000) / budget;
        if (predicted < budget) {
#pragma unroll
            for (int k = 0; k < 5; k++)
                th[k] = (int8_t)max(th[k] - 1, 0);
            final_ = 0;
        } else {
#pragma unroll
            for (int k = 0; k < 5; k++)
                th[k] = th[k] == 0 ? 0 : (int8_t)min(th[k] + 1, 100);
            final_ = 1;
        }
        if (iteration == 0)
            initial = final_;
        iteration++;
    }

    /* DeriveSearchMethod: the order of the equality tests (:1360-1392); the LCU's record gets mode, clamped score and cost */
    uint32_t bdp = 0, md = 0;
    for (int n = t; n < lcus; n += MDC_BUDGET_THREADS) {
        const uint32_t score = s_score[n], c = mdc_lcu_cost(s_avc[n >> 6] >> (n & 63) & 1ull, score - lo, mode, layer, interval, limit, ok);
        const int m = c == 97 ? MDC_PRED_OPEN_LOOP_1_NFL : c == 100 ? MDC_PRED_OPEN_LOOP : c == 106 ? MDC_LIGHT_OPEN_LOOP : c == 110 ? MDC_OPEN_LOOP :
                      c == 123 ? MDC_LIGHT_BDP : c == 129 ? MDC_BDP : c == 138 ? MDC_AVC : c == 122 ? MDC_LIGHT_AVC : layer == 0 ? MDC_FULL84 : MDC_FULL85;
        const bool is_bdp = m == MDC_LIGHT_BDP || m == MDC_BDP;
        bdp |= is_bdp, md |= !is_bdp;
        SvtAmdMdcLcu &o = J.lcu[n];
        o.lcu_md_mode = (uint8_t)m, o.lcu_score = score;
        *(uint32_t *)&o.lcu_cost = c; /* the cost and its three pad bytes */
    }
    bdp = mdc_block_sum(bdp, red), md = mdc_block_sum(md, red);
    if (t == 0) { /* bytes 8..47 of the picture record */
        P.adp_depth_sensitive_picture_class = (uint8_t)sens, P.adp_refinement_mode = (uint8_t)mode, P.number_of_segments = (uint8_t)nseg, P.pad0 = 0;
        P.budget = budget, P.predicted_cost = predicted, P.lcu_min_score = lo, P.lcu_max_score = hi;
#pragma unroll
        for (int k = 0; k < 7; k++)
            P.score_th[k] = (int8_t)th[k], P.interval_cost[k] = (uint8_t)interval[k];
        P.iterations = (uint8_t)iteration, P.bdp_present = bdp != 0, P.md_present = md != 0;
        P.pad[0] = 0, P.pad[1] = 0, P.pad[2] = 0;
    }
}

/* ---------------------------------------------------------------- the leaf list ---------------------------------------------------------------- */

#include "mdc_units.h"
/* the unit EbHevcMdcRefinement's Pm1 arm marks: cuIndex - 1 - ParentCUIndex[cuIndex] - the parent, but for unit 64, whose table entry (36) leads to unit 27 */
__device__ __forceinline__ int mdc_pm1_target(int cu, int parent) { return cu == 64 ? 27 : parent; }

/* the refinement levels (Codec/EbModeDecisionConfiguration.h): Predicted, Predicted + 1 .. + 3, Predicted - 1 .. - 3 */
enum { MDC_P = 1, MDC_PP1 = 2, MDC_PP2 = 4, MDC_PP3 = 8, MDC_PM1 = 16, MDC_PM2 = 32, MDC_PM3 = 64 };
/* the level a predicted unit of `depth` is refined with (EbHevcRefinementPredictionLoop :436): ndpRefinementLevel of the LCU's method and the picture's layer,
 * less the + arm that would reach the 8x8 units under cu8x8Mode 1 */
__device__ __forceinline__ int mdc_level(int md_mode, int layer, int depth, int cu8)
{
    int level = MDC_P;
    if (md_mode == MDC_OPEN_LOOP) /* NdpRefinementLevelNref */
        level = depth == 0 ? (layer < 3 ? MDC_P + MDC_PP1 + MDC_PP2 : MDC_P + MDC_PP1) : depth == 3 ? MDC_P + MDC_PM1 : MDC_P + MDC_PP1;
    else if (md_mode == MDC_LIGHT_OPEN_LOOP) { /* NdpRefinementLevelFast */
        if (depth == 3)
            level = MDC_P + MDC_PM1;
        else if (layer == 0)
            level = depth == 0 ? MDC_P + MDC_PP1 + MDC_PP2 : MDC_P + MDC_PP1;
        else if (layer < 3)
            level = depth == 0 ? MDC_P : MDC_P + MDC_PP1;
        else
            level = MDC_P;
    }
    if (cu8 == 1) {
        if ((level & MDC_PP1) && depth == 2)
            level -= MDC_PP1;
        else if ((level & MDC_PP2) && depth == 1)
            level -= MDC_PP2;
        else if ((level & MDC_PP3) && depth == 0)
            level -= MDC_PP3;
    }
    return level;
}
/* the lowest level EbHevcRefinementPredictionLoop finds in `level`: it looks in the order Pp3, Pp2, Pp1, P, Pm1, Pm2, Pm3 */
__device__ __forceinline__ int mdc_lowest(int level)
{
    return level & MDC_PP3 ? MDC_PP3 : level & MDC_PP2 ? MDC_PP2 : level & MDC_PP1 ? MDC_PP1 : level & MDC_P ? MDC_P : level & MDC_PM1 ? MDC_PM1 : level & MDC_PM2 ? MDC_PM2 :
           level & MDC_PM3 ? MDC_PM3 : 0;
}

/* entry d of a table by depth: selects - an index the compiler cannot resolve would put the table into scratch memory */
__device__ __forceinline__ int mdc_pick(const int (&a)[4], int d) { return d <= 0 ? a[0] : d == 1 ? a[1] : d == 2 ? a[2] : a[3]; }

/* what EbHevcMdcRefinement (:82) leaves in selected / stop of unit cu after it ran for every predicted unit (the set `root`), in gather form.  Every level
 * holds P, so no call clears a mark and the marks are the OR over the calls in any order.  level / lowest: by depth of the predicted unit */
__device__ __forceinline__ void mdc_refined(int cu, const MdcUnit &u, const MdcSet &root, const int (&level)[4], const int (&lowest)[4], bool any2, bool any3, bool &selected,
                                            bool &stop)
{
    const int d = u.depth;
    selected = false, stop = false;
    if (mdc_in(root, cu)) /* the predicted unit itself: selected by the loop; P stops it when it is the lowest level */
        selected = true, stop = mdc_pick(lowest, d) == MDC_P;
    if (d >= 1 && mdc_in(root, u.parent) && (mdc_pick(level, d - 1) & MDC_PP1))
        selected = true, stop |= mdc_pick(lowest, d - 1) == MDC_PP1;
    if (d >= 2 && mdc_in(root, u.grand) && (mdc_pick(level, d - 2) & MDC_PP2))
        selected = true, stop |= mdc_pick(lowest, d - 2) == MDC_PP2;
    if (d == 3 && mdc_in(root, 0) && (level[0] & MDC_PP3))
        selected = true, stop |= lowest[0] == MDC_PP3;
    if (d < 3 && (mdc_pick(level, d + 1) & MDC_PM1)) { /* a predicted child */
        const int step = d == 0 ? 21 : d == 1 ? 5 : 1;
        for (int q = 0; q < 4; q++) {
            const int c = cu + 1 + q * step;
            if (mdc_in(root, c) && mdc_pm1_target(c, cu) == cu)
                selected = true, stop |= mdc_pick(lowest, d + 1) == MDC_PM1;
        }
    }
    if (cu == 27 && mdc_in(root, 64) && (level[1] & MDC_PM1)) /* ParentCUIndex[64] */
        selected = true, stop |= lowest[1] == MDC_PM1;
    if (cu == 0 && any2 && (level[2] & MDC_PM2))
        selected = true, stop |= lowest[2] == MDC_PM2;
    if (d == 1 && any3 && (level[3] & MDC_PM2))
        selected = true, stop |= lowest[3] == MDC_PM2;
    if (cu == 0 && any3 && (level[3] & MDC_PM3))
        selected = true, stop |= lowest[3] == MDC_PM2; /* as written (:232): the Pm3 arm tests Pm2 */
}

/* mvBitTable (Codec/EbModeDecisionConfiguration.h:108) as md_logic.h's md_mv_bits has it: a 3 x 3 core plus 2 bits (1 << 16) per doubling of either component beyond 2 */
__device__ __forceinline__ uint32_t mdc_sel3(int i, uint32_t a, uint32_t b, uint32_t c) { return i <= 0 ? a : i == 1 ? b : c; }
__device__ __forceinline__ uint32_t mdc_mv_bits(int x, int y)
{
    const int row = min(x, 2), col = min(y, 2);
    const uint32_t core = mdc_sel3(row, mdc_sel3(col, 73744, 128728, 203592), mdc_sel3(col, 130975, 178780, 253644), mdc_sel3(col, 202683, 253623, 321933));
    const int lx = x >= 4 ? 30 - __builtin_clz((unsigned)x) : 0, ly = y >= 4 ? 30 - __builtin_clz((unsigned)y) : 0;
    return core + 65536u * (uint32_t)(lx + ly);
}

/* grid (LCUs / 4, pictures): one wave per LCU */
__global__ __launch_bounds__(256) void k_mdc_leaves(const MdcJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[4][176]; /* bytes 0..175 of the wave's record */
    const MdcJobDev &J = jobs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int lcus = lcus_w * lcus_h, lcu = (int)blockIdx.x * 4 + wave;
    const bool active = lcu < lcus;
    const int n = active ? lcu : lcus - 1; /* a wave past the last LCU computes the last one again and stores nothing */
    const int ox = n % lcus_w * 64, oy = n / lcus_w * 64;
    const int layer = J.layer;
    SvtAmdMdcLcu &O = J.lcu[n];
    const int md_mode = __builtin_amdgcn_readfirstlane((int)O.lcu_md_mode), aura = O.aura_status, avc = O.avc_partitioning; /* k_mdc_lcu's and k_mdc_budget's, kept */

    /* lane b: units b and 64 + b */
    const int cu0 = b, cu1 = b < 21 ? 64 + b : 84;
    const MdcUnit u0 = mdc_unit(cu0), u1 = mdc_unit(cu1);
    /* rasterScanCuValidity */
    const bool v0 = ox + u0.x + (64 >> u0.depth) <= width && oy + u0.y + (64 >> u0.depth) <= height;
    const bool v1 = b < 21 && ox + u1.x + (64 >> u1.depth) <= width && oy + u1.y + (64 >> u1.depth) <= height;

    /* the method of the LCU: a fixed list, the predicted open-loop list, or none */
    int fixed = 0; /* the EB_LCU_DEPTH_MODE of a fixed list */
    bool open_loop = false;
    if (J.depth_mode == MDC_PICT_LCU_SWITCH) {
        if (md_mode == MDC_FULL85 || md_mode == MDC_FULL84 || md_mode == MDC_AVC || md_mode == MDC_LIGHT_AVC)
            fixed = md_mode;
        else
            open_loop = md_mode != MDC_BDP && md_mode != MDC_LIGHT_BDP;
    } else if (J.depth_mode == MDC_PICT_FULL85 || J.depth_mode == MDC_PICT_FULL84)
        fixed = J.depth_mode == MDC_PICT_FULL85 ? MDC_FULL85 : MDC_FULL84;

    bool sel0 = false, sel1 = false, stop0 = false, stop1 = false, pred64 = false;
    if (fixed) { /* Forward85 / 84 / 8x816x16 / 16x16CuToModeDecisionLCU: the units from a first depth on, the walk stopping at a last depth */
        const int first = fixed == MDC_FULL85 ? 0 : fixed == MDC_FULL84 ? 1 : 2, last = fixed == MDC_LIGHT_AVC ? 2 : 3;
        sel0 = u0.depth >= first, stop0 = sel0 && u0.depth >= last;
        sel1 = u1.depth >= first, stop1 = sel1 && u1.depth >= last;
    } else if (open_loop) { /* EarlyModeDecisionLcu: workgroup-divergent, wave-uniform */
        /* EbHevcPredictionPartitionLoop (:903): lane r < 21 holds the cost of the 64x64, 32x32 or 16x16 unit r of the ME records (raster) */
        const int start = layer == 0 ? 1 : 0;
        const int r = b < 21 ? b : 0, rdepth = r == 0 ? 0 : r < 5 ? 1 : 2;
        const int rx = r == 0 ? 0 : r < 5 ? ((r - 1) & 1) * 32 : ((r - 5) & 3) * 16, ry = r == 0 ? 0 : r < 5 ? ((r - 1) >> 1) * 32 : ((r - 5) >> 2) * 16;
        const bool rvalid = ox + rx + (64 >> rdepth) <= width && oy + ry + (64 >> rdepth) <= height;
        const SvtAmdMeCuResult &M = J.me[n].pu[r];
        const int dir = M.direction[0];
        const int ax0 = min(abs((int)M.x_mv_l0), 499), ay0 = min(abs((int)M.y_mv_l0), 499), ax1 = min(abs((int)M.x_mv_l1), 499), ay1 = min(abs((int)M.y_mv_l1), 499);
        /* MdcInterCuRate (:307) */
        const unsigned long long rate = dir == 1 ? 86440ull + 23196ull + mdc_mv_bits(ax1, ay1) :
                                        dir == 2 ? 86440ull + 46392ull + mdc_mv_bits(ax0, ay0) + (unsigned long long)mdc_mv_bits(ax1, ay1) :
                                                   86440ull + 23196ull + mdc_mv_bits(ax0, ay0);
        const unsigned long long lambda = J.lambda;
        unsigned long long cost = (unsigned long long)(uint32_t)(M.distortion[0] << 8) + ((lambda * rate + (1ull << 22)) >> 23); /* (:1025): the shift is 32 bits wide */
        if (rdepth < start)
            cost = 0xFFFFFFFFull; /* earlyCost = ~0u (:1050) */
        const unsigned long long rate0 = (lambda * J.split_bits[0] + (1ull << 22)) >> 23, rate1 = (lambda * J.split_bits[1] + (1ull << 22)) >> 23;
        /* EbHevcMdcInterDepthDecision (:715).  The counters run as written: groupOf8x8BlocksCount is EbHevcIncrementalCount of a 16x16 unit - 4 at the fourth
         * unit of a 32x32 quadrant, where GROUP_OF_4_16x16_BLOCKS holds as well - and every VALID such unit runs the 16 -> 32 decision and counts one
         * group of 16x16 units; an invalid unit is skipped and counts nothing.  Lane q < 4 decides quadrant q */
        const int q = b & 3, fourth = 5 + ((q >> 1) * 2 + 1) * 4 + (q & 1) * 2 + 1; /* raster index of the quadrant's bottom-right 16x16 unit */
        const unsigned long long c_two = __shfl(cost, fourth), c_left = __shfl(cost, fourth - 1), c_top = __shfl(cost, fourth - 4), c_top_left = __shfl(cost, fourth - 5);
        const unsigned long long c_one = __shfl(cost, 1 + q);
        const bool fourth_valid = __shfl((int)rvalid, fourth) != 0;
        bool split32 = true; /* earlySplitFlag of the 32x32 unit */
        unsigned long long cost32 = c_one;
        if (fourth_valid) {
            const unsigned long long n_cost = c_one + rate0, n1_cost = c_two + c_left + c_top + c_top_left + rate1;
            split32 = !(n_cost <= n1_cost), cost32 = n_cost <= n1_cost ? n_cost : n1_cost;
        }
        const uint32_t groups16 = (uint32_t)__popcll(__ballot(b < 4 && fourth_valid)); /* groupOf16x16BlocksCount when the last 16x16 unit has been looked at */
        /* the 32 -> 64 decision runs at the unit where the count reaches 4: the last 16x16 unit of a complete LCU, never before (the count is 3 at most until
         * then) and never after (the 8x8 units behind it are outside the depth range) */
        const unsigned long long c64 = __shfl(cost, 0);
        const unsigned long long sum32 = __shfl(cost32, 0) + __shfl(cost32, 1) + __shfl(cost32, 2) + __shfl(cost32, 3);
        bool split64 = true;
        if (groups16 == 4)
            split64 = !(c64 + rate0 <= sum32 + rate1);
        /* EbHevcRefinementPredictionLoop (:436): the predicted units - valid, earlySplitFlag clear, below no predicted unit.  earlySplitFlag is depth < 2 (:957)
         * but where a decision cleared it */
        const unsigned long long m_split32 = __ballot(b < 4 && split32); /* bit q */
        const bool es0 = u0.depth == 0 ? split64 : u0.depth == 1 ? (m_split32 >> ((cu0 - 1) / 21) & 1ull) != 0 : false;
        const bool es1 = u1.depth == 1 ? (m_split32 >> 3 & 1ull) != 0 : false; /* unit 64 is the only one above 63 that is no 16x16 or 8x8 unit */
        const MdcSet cand = mdc_set(v0 && !es0, v1 && !es1);
        const MdcSet root = mdc_set(v0 && !es0 && !mdc_in(cand, u0.parent) && !mdc_in(cand, u0.grand) && !mdc_in(cand, u0.great),
                                    v1 && !es1 && !mdc_in(cand, u1.parent) && !mdc_in(cand, u1.grand) && !mdc_in(cand, u1.great));
        pred64 = mdc_in(root, 0);
        int level[4], lowest[4];
#pragma unroll
        for (int d = 0; d < 4; d++)
            level[d] = mdc_level(md_mode, layer, d, J.cu8), lowest[d] = mdc_lowest(level[d]);
        const bool root0 = mdc_in(root, cu0), root1 = b < 21 && mdc_in(root, cu1);
        const bool any2 = (__ballot(root0 && u0.depth == 2) | __ballot(root1 && u1.depth == 2)) != 0;
        const bool any3 = (__ballot(root0 && u0.depth == 3) | __ballot(root1 && u1.depth == 3)) != 0;
        mdc_refined(cu0, u0, root, level, lowest, any2, any3, sel0, stop0);
        mdc_refined(cu1, u1, root, level, lowest, any2, any3, sel1, stop1);
    }
    /* EbHevcForwardCuToModeDecision (:586) and the fixed walks alike: a unit enters the list when it is valid, no valid ancestor stopped the walk, and it is an
     * 8x8 unit, stopped or selected; it carries splitFlag 1 unless it is an 8x8 unit or stopped */
    const MdcSet halt = mdc_set(v0 && stop0, v1 && stop1);
    const bool list = fixed || open_loop;
    const bool e0 = list && v0 && !mdc_in(halt, u0.parent) && !mdc_in(halt, u0.grand) && !mdc_in(halt, u0.great) && (u0.depth == 3 || stop0 || sel0);
    const bool e1 = list && v1 && !mdc_in(halt, u1.parent) && !mdc_in(halt, u1.grand) && !mdc_in(halt, u1.great) && (u1.depth == 3 || stop1 || sel1);
    const MdcSet emitted = mdc_set(e0, e1);
    const int count_lo = __popcll(emitted.lo), count = count_lo + __popcll(emitted.hi);

    /* the record's bytes 0..175 in LDS: zeroed, the list scattered to its places, then stored as 44 words */
    uint8_t *rec = s_rec[wave];
    if (b < 44)
        ((uint32_t *)rec)[b] = 0;
    __syncthreads();
    if (e0) {
        const int at = __popcll(emitted.lo & ((1ull << b) - 1ull));
        rec[1 + at] = (uint8_t)cu0, rec[86 + at] = u0.depth < 3 && !stop0;
    }
    if (e1) {
        const int at = count_lo + __popcll(emitted.hi & ((1ull << b) - 1ull));
        rec[1 + at] = (uint8_t)cu1, rec[86 + at] = u1.depth < 3 && !stop1;
    }
    if (b == 0)
        rec[0] = (uint8_t)count, rec[171] = (uint8_t)md_mode, rec[172] = (uint8_t)aura, rec[173] = pred64, rec[174] = (uint8_t)avc;
    __syncthreads();
    if (active && b < 44)
        ((uint32_t *)&O)[b] = ((const uint32_t *)rec)[b];
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

static int g_mdc_stages = 7; /* svt_amd_debug_md_config_stages */
extern "C" void svt_amd_debug_md_config_stages(int mask) { g_mdc_stages = mask; }

extern "C" size_t svt_amd_md_config_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    switch (which) {
    case SVT_AMD_MDC_LCU:
        return (size_t)svt_amd_lcu_count(luma_width, luma_height) * sizeof(SvtAmdMdcLcu);
    case SVT_AMD_MDC_PICTURE:
        return sizeof(SvtAmdMdcPic);
    }
    return 0;
}

extern "C" int svt_amd_md_config_batch_launch(SvtAmdContext *ctx, const SvtAmdMdcJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                              const SvtAmdMdcArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    SvtAmdBatchGeometry g; /* SVT_AMD_MDC_MAX_LCUS: the bound up to which the signed product of the budgeting loop (:1522) is defined */
    SVT_AMD_TRY(svt_amd_batch_geometry(__func__, ctx, luma_width, luma_height, SVT_AMD_MDC_MAX_LCUS, true, &g));
    const auto [w, h, wl, hl, lcus, groups, cap_lcus, cap_groups] = g;
    if (!out->lcu || !out->picture)
        SVT_AMD_BAD("%s: job 0: there is no %s array", __func__, out->lcu ? "picture" : "lcu");
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdMdcJob &j = jobs[i];
        if (!j.stats || !j.detect || !j.sbo_lcu || !j.sbo_pic || !j.pic_detect || !j.noise_pic)
            SVT_AMD_BAD("%s: job %d has no %s", __func__, i, !j.stats ? "block statistics" : !j.detect ? "detector records" : !j.sbo_lcu ? "source-ops LCU records" :
                        !j.sbo_pic ? "source-ops picture record" : !j.pic_detect ? "detector picture record" : "noise picture record");
        if (j.slice_type != 1 && j.slice_type != 2)
            SVT_AMD_BAD("%s: job %d: slice type %d (1 P or 2 B: the I-picture arm is not built)", __func__, i, j.slice_type);
        if (j.temporal_layer_index > 5 || j.hierarchical_levels > 5 || j.resolution_class > 3 || j.depth_mode > 5 || j.qp > 51)
            SVT_AMD_BAD("%s: job %d: temporal layer %d, hierarchical levels %d, resolution class %d, depth mode %d, QP %d", __func__, i, j.temporal_layer_index,
                        j.hierarchical_levels, j.resolution_class, j.depth_mode, j.qp);
        if (!j.me) /* the records resident in the slot */
            SVT_AMD_TRY(svt_amd_batch_slot_records(__func__, ctx, i, j.cur_slot, BATCH_REC_ME, w, h));
    }

    MdcJobDev *d_tab;
    uint8_t *d_scratch; /* per picture: a score word, then a flag byte per LCU */
    const size_t pic_scratch = (size_t)((cap_lcus + 3) & ~3) * 5;
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_MDC, sizeof(MdcJobDev), pic_scratch * SVT_AMD_MAX_BATCH, (void **)&d_tab, (void **)&d_scratch));
    static thread_local MdcJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    SvtAmdRecordsBinder bind;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdMdcJob &j = jobs[i];
        MdcJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        d.me = j.me;
        if (!j.me)
            SVT_AMD_TRY(svt_amd_batch_bind_records(ctx, &bind, j.cur_slot, SLOT_ME, (const void **)&d.me));
        d.stats = j.stats, d.detect = j.detect, d.sbo_lcu = j.sbo_lcu, d.sbo_pic = j.sbo_pic, d.pic_detect = j.pic_detect, d.noise_pic = j.noise_pic;
        d.stationary = j.stationary_edge;
        d.lcu = out->lcu + (size_t)i * lcus;
        d.pic = out->picture + i;
        d.score = (uint32_t *)(d_scratch + (size_t)i * pic_scratch);
        d.avc = d_scratch + (size_t)i * pic_scratch + (size_t)((cap_lcus + 3) & ~3) * 4;
        d.lambda = j.lambda_sad, d.split_bits[0] = j.split_flag_bits[0], d.split_bits[1] = j.split_flag_bits[1];
        d.slice = j.slice_type, d.layer = j.temporal_layer_index, d.hier = j.hierarchical_levels, d.is_ref = j.is_used_as_reference != 0;
        d.depth_mode = j.depth_mode, d.enc_mode = j.enc_mode, d.cls = j.resolution_class, d.qp = j.qp, d.pan = j.is_pan != 0, d.tilt = j.is_tilt != 0;
        d.ndth = j.noise_detection_th, d.homog = j.homogeneity_percentage, d.fr30 = j.frame_rate_30 != 0, d.cu8 = j.cu8x8_mode, d.avg_int = j.average_intensity;
        d.ref_int[0] = j.ref_average_intensity[0], d.ref_int[1] = j.ref_average_intensity[1];
        d.ref_skip[0] = j.ref_penalize_skip[0] != 0, d.ref_skip[1] = j.ref_penalize_skip[1] != 0;
    }
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(MdcJobDev) * (size_t)num_jobs));
    /* the stages are ordered on the lane, and the scratch is stored into, never added to: a batch queued behind this one overwrites it only after this one's
     * budget kernel has read it, and there is nothing to zero */
    const size_t budget_lds = (size_t)((lcus + 1) & ~1) * 4 + (size_t)((lcus + 63) / 64) * 8;
    if (g_mdc_stages & 1)
        hipLaunchKernelGGL(k_mdc_lcu, dim3((unsigned)groups, (unsigned)num_jobs), dim3(256), 0, st, (const MdcJobDev *)d_tab, w, h, wl, hl);
    if (g_mdc_stages & 2)
        hipLaunchKernelGGL(k_mdc_budget, dim3((unsigned)num_jobs), dim3(MDC_BUDGET_THREADS), budget_lds, st, (const MdcJobDev *)d_tab, w, h, wl, hl);
    if (g_mdc_stages & 4)
        hipLaunchKernelGGL(k_mdc_leaves, dim3((unsigned)groups, (unsigned)num_jobs), dim3(256), 0, st, (const MdcJobDev *)d_tab, w, h, wl, hl);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
