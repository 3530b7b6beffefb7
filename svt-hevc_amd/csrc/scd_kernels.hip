/*
 * scd_kernels.hip - SceneTransitionDetector of the picture decision (Codec/EbPictureDecisionProcess.c:73-258) in the batched, stream-ordered shape of
 * irc_kernels.hip (include/svt_hevc_amd.h "Batched scene-transition detection"): the jobs of a batch are CONSECUTIVE CALLS of the detector, the
 * per-job pointers come from a descriptor table in device memory - the caller's SvtAmdScdJob records as they are - and nothing is copied to the host.  The rules
 * are scd_logic.h's, the text tools/scd_logic_check.c compiles for the host; tests/scd_numpy.py restates them from the reference.
 *   k_scd_ahd       grid (regions, jobs), 256 threads, a thread per bin: |cur - past| of the bin in the luma, the Cb and the Cr histogram of the region - three
 *                   pairs of coalesced dword loads, the chroma pair of a region 2 KB contiguous - reduced by wave shuffles and four words of LDS per plane;
 *                   the three sums are STORED into out.ahd.  The workgroup of region 0 stores the 0 of the entries beyond the regions.  Parallel over the batch.
 *   k_scd_decide    ONE workgroup of one wave, a lane per region, a loop over the jobs in order.  The lane keeps its region's three running averages in
 *                   registers from job to job; the two counts are population counts of wave ballots, so the reset flag and the return value are
 *                   wave-uniform without a broadcast.  Lanes 0..15 store their part of state[i] and region_class, lane 0 the rest of both records.  Loading
 *                   the inputs of job i + 1 (three sums, three intensity bytes, two variances behind two pointers) before job i is decided was measured and is
 *                   slower (64 jobs: 56.7 against 53.1 us for this kernel alone, profiles/r42_c): the loop loads what it decides.
 * Every array is written by one kernel only; no atomics, nothing to zero.  Bound: latency - 12,288 histogram words a job in the first stage, a chain of
 * dependent steps a job in the second.
 */
#include "pa_batch.h"
#define SCD_FN __host__ __device__ static inline
#include "scd_logic.h"

static_assert(sizeof(SvtAmdScdJob) == 72 && sizeof(SvtAmdScdPic) == 24 && sizeof(SvtAmdScdState) == 196, "scene-detection records");
static_assert(offsetof(SvtAmdScdPic, region_class) == 8 && offsetof(SvtAmdScdState, ahd_running_avg_cb) == 64 && offsetof(SvtAmdScdState, reset_running_avg) == 192,
              "scene-detection record layout");
static_assert(SVT_AMD_SCD_MAX_REGIONS == SCD_MAX_REGIONS && SVT_AMD_SCD_CLASS_SCENE == SCD_SCENE && SVT_AMD_SCD_CLASS_FLASH == SCD_FLASH, "scd_logic.h");
#define SCD_AHD_WORDS (SCD_MAX_REGIONS * 3)

__device__ __forceinline__ uint32_t scd_wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v += (uint32_t)__shfl_xor(v, o);
    return v;
}

/* grid (regions, jobs): a thread per bin */
__global__ __launch_bounds__(SCD_BINS) void k_scd_ahd(const SvtAmdScdJob *__restrict__ jobs, uint32_t *__restrict__ ahd, int regions)
{
    __shared__ uint32_t red[3][SCD_BINS / 64];
    const SvtAmdScdJob &J = jobs[blockIdx.y];
    const int r = blockIdx.x, t = threadIdx.x;
    const size_t luma = (size_t)r * SCD_BINS + t, chroma = (size_t)r * 2 * SCD_BINS + t;
    uint32_t y = scd_abs_diff(J.cur_histogram[luma], J.past_histogram[luma]);
    uint32_t cb = scd_abs_diff(J.cur_chroma_histogram[chroma], J.past_chroma_histogram[chroma]);
    uint32_t cr = scd_abs_diff(J.cur_chroma_histogram[chroma + SCD_BINS], J.past_chroma_histogram[chroma + SCD_BINS]);
    y = scd_wave_sum(y), cb = scd_wave_sum(cb), cr = scd_wave_sum(cr);
    if ((t & 63) == 0)
        red[0][t >> 6] = y, red[1][t >> 6] = cb, red[2][t >> 6] = cr;
    __syncthreads();
    uint32_t *o = ahd + (size_t)blockIdx.y * SCD_AHD_WORDS;
    if (t < 3)
        o[r * 3 + t] = red[t][0] + red[t][1] + red[t][2] + red[t][3];
    if (r == 0 && t < (SCD_MAX_REGIONS - regions) * 3) /* the entries no region has */
        o[regions * 3 + t] = 0;
}

/* what one lane reads for one job */
struct ScdInputs { uint32_t ahd[3], past, cur, future, cur_variance, past_variance; };
__device__ __forceinline__ ScdInputs scd_load(const SvtAmdScdJob *__restrict__ jobs, const uint32_t *ahd, int i, int lane, bool active)
{
    const SvtAmdScdJob &J = jobs[i];
    ScdInputs in = {};
    in.cur_variance = J.cur_detect->pic_avg_variance, in.past_variance = J.past_detect->pic_avg_variance;
    if (active) {
        const uint32_t *a = ahd + (size_t)i * SCD_AHD_WORDS + lane * 3;
        in.ahd[0] = a[0], in.ahd[1] = a[1], in.ahd[2] = a[2];
        in.past = J.past_region_average[lane], in.cur = J.cur_region_average[lane], in.future = J.future_region_average[lane];
    }
    return in;
}

/* one workgroup of one wave: lane = region wi * rh + hi */
__global__ __launch_bounds__(64) void k_scd_decide(const SvtAmdScdJob *__restrict__ jobs, int num_jobs, int w, int h, int rw, int rh, int scd_mode,
                                                   const SvtAmdScdState *state_in, SvtAmdScdPic *__restrict__ pictures, const uint32_t *ahd,
                                                   SvtAmdScdState *__restrict__ states)
{
    const int lane = threadIdx.x, regions = rw * rh;
    const bool active = lane < regions;
    const uint32_t r = active ? (uint32_t)lane : 0u, wi = r / (uint32_t)rh, hi = r - wi * (uint32_t)rh;
    /* NUM64x64INPIC of this lane's iteration: the threshold is 3000 or 4500 times it */
    const uint32_t units = scd_region_threshold((uint32_t)w, (uint32_t)h, (uint32_t)rw, (uint32_t)rh, wi, hi, 1u);
    const uint32_t vote = scd_vote_threshold((uint32_t)regions, (uint32_t)scd_mode);
    uint32_t avg[3] = {0, 0, 0}, reset = 1; /* PictureDecisionContextCtor (:63-68) */
    if (state_in) {
        if (active)
            avg[0] = state_in->ahd_running_avg[lane], avg[1] = state_in->ahd_running_avg_cb[lane], avg[2] = state_in->ahd_running_avg_cr[lane];
        reset = state_in->reset_running_avg != 0;
    }
    for (int i = 0; i < num_jobs; i++) {
        const ScdInputs in = scd_load(jobs, ahd, i, lane, active);
        const uint32_t th = scd_scene_th(in.cur_variance, in.past_variance) * units;
        uint32_t cls = SCD_NONE;
        if (active)
            cls = scd_region(in.ahd, avg, reset, th, th / 4u, in.past, in.cur, in.future);
        const uint32_t abrupt = (uint32_t)__popcll(__ballot(cls >= SCD_FLASH)), scene = (uint32_t)__popcll(__ballot(cls == SCD_SCENE));
        reset = abrupt >= vote;
        SvtAmdScdState &s = states[i];
        SvtAmdScdPic &p = pictures[i];
        if (lane < SCD_MAX_REGIONS) { /* every byte of both records is stored; avg is 0 in a lane without a region */
            s.ahd_running_avg[lane] = avg[0], s.ahd_running_avg_cb[lane] = avg[1], s.ahd_running_avg_cr[lane] = avg[2];
            p.region_class[lane] = (uint8_t)cls;
        }
        if (lane == 0) {
            s.reset_running_avg = (uint8_t)reset, s.pad[0] = 0, s.pad[1] = 0, s.pad[2] = 0;
            p.scene_change = scene >= vote, p.reset_running_avg = (uint8_t)reset, p.abrupt_regions = (uint8_t)abrupt, p.scene_regions = (uint8_t)scene;
            p.region_count_threshold = (uint8_t)vote, p.pad[0] = 0, p.pad[1] = 0, p.pad[2] = 0;
        }
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

static bool scd_regions_ok(int regions_w, int regions_h) { return regions_w >= 1 && regions_w <= 4 && regions_h >= 1 && regions_h <= 4; }

extern "C" size_t svt_amd_scene_detect_bytes(int which, int regions_w, int regions_h)
{
    if (!scd_regions_ok(regions_w, regions_h))
        return 0;
    switch (which) {
    case SVT_AMD_SCD_PICTURE:
        return sizeof(SvtAmdScdPic);
    case SVT_AMD_SCD_AHD:
        return SCD_AHD_WORDS * sizeof(uint32_t);
    case SVT_AMD_SCD_STATE:
        return sizeof(SvtAmdScdState);
    }
    return 0;
}

static int g_scd_stages = 3; /* svt_amd_debug_scene_detect_stages */
extern "C" void svt_amd_debug_scene_detect_stages(int mask) { g_scd_stages = mask; }

extern "C" int svt_amd_scene_detect_batch_launch(SvtAmdContext *ctx, const SvtAmdScdJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height,
                                                 int regions_w, int regions_h, int scd_mode, const SvtAmdScdState *d_state_in, const SvtAmdScdArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    /* what belongs to the whole batch names no job; a size above the bound is refused in the words the batched entries share ("job 0: a picture of ...") */
    if (!scd_regions_ok(regions_w, regions_h))
        SVT_AMD_BAD("%s: %d x %d regions (1..4 each)", __func__, regions_w, regions_h);
    if (scd_mode < 1 || scd_mode > 2)
        SVT_AMD_BAD("%s: scd_mode %d (1..2)", __func__, scd_mode);
    if (luma_width < 8 || luma_height < 8)
        SVT_AMD_BAD("%s: a picture of %dx%d (at least 8x8)", __func__, luma_width, luma_height);
    SvtAmdBatchGeometry g;
    SVT_AMD_TRY(svt_amd_batch_geometry(__func__, ctx, luma_width, luma_height, SVT_AMD_SCD_MAX_LCUS, false, &g));
    if (!out->picture || !out->ahd || !out->state)
        SVT_AMD_BAD("%s: there is no %s array", __func__, !out->picture ? "picture" : !out->ahd ? "ahd" : "state");
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdScdJob &j = jobs[i];
        const char *missing = !j.past_histogram ? "past_histogram" : !j.cur_histogram ? "cur_histogram" : !j.past_chroma_histogram ? "past_chroma_histogram" :
                              !j.cur_chroma_histogram ? "cur_chroma_histogram" : !j.past_region_average ? "past_region_average" :
                              !j.cur_region_average ? "cur_region_average" : !j.future_region_average ? "future_region_average" :
                              !j.past_detect ? "past_detect" : !j.cur_detect ? "cur_detect" : nullptr;
        if (missing)
            SVT_AMD_BAD("%s: job %d has no %s", __func__, i, missing);
    }

    SvtAmdScdJob *d_tab;
    void *d_scratch; /* none: the first stage's sums are an output array */
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_SCD, sizeof(SvtAmdScdJob), 0, (void **)&d_tab, &d_scratch));
    hipStream_t st = svt_amd_ctx_stream(ctx);
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, jobs, sizeof(SvtAmdScdJob) * (size_t)num_jobs));
    const int regions = regions_w * regions_h, stages = g_scd_stages;
    if (stages & 1)
        hipLaunchKernelGGL(k_scd_ahd, dim3((unsigned)regions, (unsigned)num_jobs), dim3(SCD_BINS), 0, st, (const SvtAmdScdJob *)d_tab, out->ahd, regions);
    if (stages & 2)
        hipLaunchKernelGGL(k_scd_decide, dim3(1), dim3(64), 0, st, (const SvtAmdScdJob *)d_tab, num_jobs, g.w, g.h, regions_w, regions_h, scd_mode, d_state_in,
                           out->picture, (const uint32_t *)out->ahd, out->state);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
