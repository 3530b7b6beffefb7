/*
 * side_kernels.hip - the batched, stream-ordered form of the three per-picture side results of the front half (include/svt_hevc_amd.h
 * "Batched side statistics"): block statistics + AC energy, the luma region histograms, and the collocated zero-motion SAD.
 * The arithmetic is that of pa_kernels.hip / ois_kernels.hip (k_pa_block_stats, k_sbo_ac_energy, k_pa_histogram, k_pa_finish, k_zz_sad), which stay as
 * they are behind the blocking single-picture entries; what is new is the shape: the picture is a grid dimension, the per-picture plane and output
 * pointers come from a descriptor table in device memory (as for k_pack_* and the prep / ME / OIS batches), and nothing is copied to the host.
 *   k_side_luma         ComputeBlockMeanComputeVariance (Codec/EbPictureAnalysisProcess.c:1646) AND CalculateAcEnergy (Codec/EbSourceBasedOperationsProcess.c:302)
 *                       from ONE read of the full-resolution plane: grid (LCUs, pictures), one wave per LCU, a lane per 8x8 block; the lane loads its eight
 *                       8-byte rows once - the even rows feed v_sad_u8 / v_dot4_u32_u8 (ComputeSubMean8x8_SSE2_INTRIN), all eight the register Hadamard
 *                       (Compute8x8Satd_U8, C_DEFAULT/EbPictureOperators_C.c:563); the 16 / 32 / 64 levels of both come from lane shuffles.
 *   k_side_hist(_finish) SubSampleLumaGeneratePixelIntensityHistogramBins (:3384) on the 1/16 pictures: grid (strips, regions, pictures).
 *   k_side_zz           ComputeDecimatedZzSad (Codec/EbMotionEstimationProcess.c:176-300) over (current, previous) 1/16 plane pairs: grid (LCUs / 4, pictures).
 * Bound: HBM - 1 B/pel for k_side_luma (the two separate kernels: 1 + 1), 1/16 B/pel for the histograms, 2/16 B/pel for the zero-motion SAD.
 */
#include "pa_batch.h"
#include <string.h>

/* where the kernels find picture i of a batch; a null pointer = that result is not wanted for the picture (a workgroup-uniform branch) */
struct SideJobDev {
    const uint8_t *full;           /* padded luma, sample (0,0): null when neither block statistics nor energies are wanted */
    const uint8_t *six, *prev_six; /* 1/16 planes of the picture and of the previous picture in display order */
    SvtAmdPaLcuStats *stats;       /* [lcus]        */
    unsigned long long *energy;    /* [lcus][5]     */
    SvtAmdZzLcu *zz;               /* [lcus]        */
    uint32_t *hist;                /* [regions][256] */
    unsigned long long *sums;      /* [regions]: context-owned scratch, zeroed by the call */
    uint8_t *region_avg;           /* [64] or null  */
    unsigned long long *total;     /* [1] or null   */
    int32_t pitch_full, pitch_six;
    int32_t pad[2];
};
static_assert(sizeof(SideJobDev) == 96, "SideJobDev layout");
#define SIDE_SUMS_BYTES ((size_t)SVT_AMD_MAX_BATCH * 64 * 8)
#define SIDE_STRIPS 16

/* 8-point Hadamard butterflies in place (pa_kernels.hip: only v[0] = the sum and the multiset of magnitudes matter) */
__device__ __forceinline__ void side_hadamard8(int *v)
{
#pragma unroll
    for (int span = 4; span > 0; span >>= 1)
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (!(i & span)) {
                const int a = v[i], b = v[i + span];
                v[i] = a + b, v[i + span] = a - b;
            }
}

__global__ __launch_bounds__(64) void k_side_luma(const SideJobDev *__restrict__ jobs, int width, int height, int lcus_w)
{
    const SideJobDev &J = jobs[blockIdx.y];
    if (!J.full)
        return;
    const int lcu = blockIdx.x, b = threadIdx.x, lx = (lcu % lcus_w) * 64, ly = (lcu / lcus_w) * 64; /* b: 8x8 block of the LCU, raster */
    const int pitch = J.pitch_full;
    const uint8_t *p = J.full + (size_t)(ly + (b >> 3) * 8) * pitch + lx + (b & 7) * 8;
    const bool complete = lx + 64 <= width && ly + 64 <= height;
    const bool want_energy = J.energy != nullptr && complete;
    /* the one read: incomplete LCUs read the slot's padded plane (68 samples right of and below the picture are valid) */
    uint2 row[8];
#pragma unroll
    for (int r = 0; r < 8; r++)
        row[r] = (!(r & 1) || want_energy) ? *(const uint2 *)(p + (size_t)r * pitch) : make_uint2(0u, 0u); /* the odd rows only feed the Hadamard */

    if (J.stats) {
        uint32_t sum = 0, sq = 0;
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
            sum = __builtin_amdgcn_sad_u8(row[r].x, 0u, sum);
            sum = __builtin_amdgcn_sad_u8(row[r].y, 0u, sum);
            sq = __builtin_amdgcn_udot4(row[r].x, row[r].x, sq, false);
            sq = __builtin_amdgcn_udot4(row[r].y, row[r].y, sq, false);
        }
        /* means with 8, means of squares with 16 fractional bits; every level above: (four children) >> 2 */
        unsigned long long m = (unsigned long long)sum << 3, s = (unsigned long long)sq << 11;
        SvtAmdPaLcuStats &o = J.stats[lcu];
        o.y_mean[21 + b] = (uint8_t)(m >> 8), o.variance[21 + b] = (uint16_t)((s - m * m) >> 16);
        /* 16x16: lanes b, b ^ 1, b ^ 8, b ^ 9 hold its four 8x8 blocks */
        unsigned long long m16 = m + __shfl_xor(m, 1), s16 = s + __shfl_xor(s, 1);
        m16 = (m16 + __shfl_xor(m16, 8)) >> 2, s16 = (s16 + __shfl_xor(s16, 8)) >> 2;
        if (!(b & 9))
            o.y_mean[5 + ((b >> 4) << 2) + ((b & 7) >> 1)] = (uint8_t)(m16 >> 8), o.variance[5 + ((b >> 4) << 2) + ((b & 7) >> 1)] = (uint16_t)((s16 - m16 * m16) >> 16);
        /* 32x32: the four 16x16 of it sit at lane offsets 2 and 16 */
        unsigned long long m32 = m16 + __shfl_xor(m16, 2), s32 = s16 + __shfl_xor(s16, 2);
        m32 = (m32 + __shfl_xor(m32, 16)) >> 2, s32 = (s32 + __shfl_xor(s32, 16)) >> 2;
        if (!(b & 27))
            o.y_mean[1 + ((b >> 5) << 1) + ((b & 7) >> 2)] = (uint8_t)(m32 >> 8), o.variance[1 + ((b >> 5) << 1) + ((b & 7) >> 2)] = (uint16_t)((s32 - m32 * m32) >> 16);
        unsigned long long m64 = m32 + __shfl_xor(m32, 4), s64 = s32 + __shfl_xor(s32, 4);
        m64 = (m64 + __shfl_xor(m64, 32)) >> 2, s64 = (s64 + __shfl_xor(s64, 32)) >> 2;
        if (b == 0)
            o.y_mean[0] = (uint8_t)(m64 >> 8), o.variance[0] = (uint16_t)((s64 - m64 * m64) >> 16), o.pad = 0;
    }

    if (!J.energy)
        return;
    unsigned long long *e = J.energy + (size_t)lcu * 5;
    if (!complete) { /* the reference's "not computed" value (Codec/EbSourceBasedOperationsProcess.c:351) */
        if (b < 5)
            e[b] = 100000000ull;
        return;
    }
    int m[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
#pragma unroll
        for (int c = 0; c < 4; c++)
            m[r][c] = (row[r].x >> (8 * c)) & 255, m[r][4 + c] = (row[r].y >> (8 * c)) & 255;
        side_hadamard8(m[r]);
    }
    uint32_t satd = 0, dc = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int col[8];
#pragma unroll
        for (int r = 0; r < 8; r++)
            col[r] = m[r][c];
        side_hadamard8(col);
#pragma unroll
        for (int r = 0; r < 8; r++)
            satd += (uint32_t)abs(col[r]);
        if (c == 0)
            dc = (uint32_t)col[0];
    }
    uint32_t s = (satd + 2) >> 2; /* Compute8x8Satd_U8: the block's rounded sum; *dcValue += m2[0][0] */
    /* the 32x32 the lane's block belongs to: lanes that differ in bits 0, 1 (x) and 3, 4 (y) */
    s += __shfl_xor(s, 1), dc += __shfl_xor(dc, 1);
    s += __shfl_xor(s, 2), dc += __shfl_xor(dc, 2);
    s += __shfl_xor(s, 8), dc += __shfl_xor(dc, 8);
    s += __shfl_xor(s, 16), dc += __shfl_xor(dc, 16);
    if (!(b & 27))
        e[1 + ((b >> 5) << 1) + ((b & 7) >> 2)] = (unsigned long long)s - (dc >> 2);
    s += __shfl_xor(s, 4), dc += __shfl_xor(dc, 4);
    s += __shfl_xor(s, 32), dc += __shfl_xor(dc, 32);
    if (b == 0)
        e[0] = (unsigned long long)s - (dc >> 2);
}

/* grid (strips, regions, pictures): rows [y0, y1) x columns [x0, x1) of the 1/16 picture; the last region of a row / column takes the remainder */
__global__ __launch_bounds__(256) void k_side_hist(const SideJobDev *__restrict__ jobs, int width, int height, int regions_w, int regions_h)
{
    const SideJobDev &J = jobs[blockIdx.z];
    if (!J.hist)
        return;
    __shared__ uint32_t bins[256];
    __shared__ unsigned long long s_sum;
    const int t = threadIdx.x, region = blockIdx.y, a = region / regions_h, b = region - a * regions_h;
    const int rw = width / regions_w, rh = height / regions_h;
    const int x0 = a * rw, x1 = a == regions_w - 1 ? width : x0 + rw, y0 = b * rh, y1 = b == regions_h - 1 ? height : y0 + rh;
    bins[t] = 0;
    if (t == 0)
        s_sum = 0;
    __syncthreads();
    const int w = x1 - x0, rows = y1 - y0, strips = gridDim.x, per = (rows + strips - 1) / strips;
    const int ys = y0 + (int)blockIdx.x * per, ye = min(ys + per, y1);
    const uint8_t *six = J.six;
    const int pitch = J.pitch_six;
    unsigned long long sum = 0;
    for (int i = t; i < (ye > ys ? (ye - ys) * w : 0); i += 256) {
        const int y = ys + i / w, x = x0 + i % w;
        const uint32_t v = six[(size_t)y * pitch + x];
        atomicAdd(&bins[v], 1u);
        sum += v;
    }
    for (int o = 32; o > 0; o >>= 1)
        sum += __shfl_xor(sum, o);
    if ((t & 63) == 0 && sum)
        atomicAdd(&s_sum, sum);
    __syncthreads();
    if (bins[t])
        atomicAdd(&J.hist[region * 256 + t], bins[t]);
    if (t == 0 && s_sum)
        atomicAdd(&J.sums[region], s_sum);
}

/* grid (regions, pictures) */
__global__ __launch_bounds__(256) void k_side_hist_finish(const SideJobDev *__restrict__ jobs, int width, int height, int regions_w, int regions_h)
{
    const SideJobDev &J = jobs[blockIdx.y];
    if (!J.hist)
        return;
    const int region = blockIdx.x, t = threadIdx.x, a = region / regions_h, b = region - a * regions_h;
    J.hist[region * 256 + t] = (J.hist[region * 256 + t] + 1u) << 4; /* bins start at 1 (InitializeBuffer_32bits ... 1) and end << 4 (:3430) */
    if (t == 0) {
        const int rw = width / regions_w, rh = height / regions_h;
        const unsigned long long w = a == regions_w - 1 ? width - a * rw : rw, h = b == regions_h - 1 ? height - b * rh : rh;
        if (J.region_avg)
            J.region_avg[region] = (uint8_t)((J.sums[region] + ((w * h) >> 1)) / (w * h));
        if (J.total)
            atomicAdd(J.total, J.sums[region] << 4);
    }
    if (region == 0 && J.region_avg && t >= regions_w * regions_h && t < 64) /* the padding of the picture's 64 bytes */
        J.region_avg[t] = 0;
}

/* grid (LCUs / 4, pictures): one wavefront per LCU; lane = (row, 4-sample group) of the 16x16 the LCU is at 1/16: one v_sad_u8 */
__global__ __launch_bounds__(256) void k_side_zz(const SideJobDev *__restrict__ jobs, int width, int height, int nlcu, int lcus_w)
{
    const SideJobDev &J = jobs[blockIdx.y];
    const int lcu = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (!J.prev_six || lcu >= nlcu)
        return;
    const int ox = (lcu % lcus_w) * 64, oy = (lcu / lcus_w) * 64;
    const int lw = min(64, width - ox), lh = min(64, height - oy);
    uint32_t sad = ~0u;
    uint8_t zz = 0xFF;
    if (lw == 64 && lh == 64) {
        const int r = lane >> 2, g = (lane & 3) << 2;
        const ptrdiff_t at = (ptrdiff_t)((oy >> 2) + r) * J.pitch_six + (ox >> 2) + g;
        uint32_t s = __builtin_amdgcn_sad_u8(*(const uint32_t *)(J.six + at), *(const uint32_t *)(J.prev_six + at), 0u);
        for (int o = 32; o > 0; o >>= 1)
            s += __shfl_xor(s, o);
        sad = s;
        zz = sad < 256 ? 0 : sad < 512 ? 3 : sad < 1024 ? 10 : sad < 2048 ? 20 : 30;
    }
    if (lane == 0) {
        const uint32_t area = (uint32_t)((lw >> 2) * (lh >> 2));
        SvtAmdZzLcu o;
        o.sad = sad, o.zz_cost = zz;
        o.non_moving_index = sad < area * 2 ? 0 : sad < area * 4 ? 10 : sad < area * 8 ? 20 : 30;
        o.pad[0] = o.pad[1] = 0;
        J.zz[lcu] = o;
    }
}

/* ---- what the batched entries share on the host (pa_batch.h) ---- */

int svt_amd_batch_header(const char *entry, const SvtAmdContext *ctx, const void *jobs, const void *out, int num_jobs)
{
    if (!ctx || !jobs || !out || num_jobs < 1 || num_jobs > SVT_AMD_MAX_BATCH)
        SVT_AMD_BAD("%s: a context, an output table and 1..%d jobs", entry, SVT_AMD_MAX_BATCH);
    return SVT_AMD_OK;
}

/* one job's picture slot: job 0 gives the batch its size (*w, *h), every job - job 0 included - has to hold a picture of that size */
int svt_amd_batch_slot(const char *entry, const SvtAmdContext *ctx, int job, int slot, int *w, int *h)
{
    const DevPicture *c = slot >= 0 && slot < ctx->num_slots ? &ctx->slots[slot] : nullptr;
    if (job == 0) {
        if (!c)
            SVT_AMD_BAD("%s: job 0: bad slot %d", entry, slot);
        *w = c->width, *h = c->height;
    }
    if (!c || !c->valid)
        SVT_AMD_BAD("%s: job %d: slot %d holds no picture", entry, job, slot);
    if (c->width != *w || c->height != *h)
        SVT_AMD_BAD("%s: pictures of different sizes in one batch (job %d: %dx%d, job 0: %dx%d)", entry, job, c->width, c->height, *w, *h);
    return SVT_AMD_OK;
}

static thread_local uint8_t seen[4096]; /* the slots this call has waited on; a context of more slots waits once per use instead */

/* the first device call of a launcher.  The entry's descriptor table (SVT_AMD_MAX_BATCH records) and, behind it, the scratch its kernels accumulate into are
 * one allocation the context owns (d_batch[which]), made at the entry's first call and freed by svt_amd_context_destroy. */
int svt_amd_batch_begin(SvtAmdContext *ctx, SvtAmdBatchEntry which, size_t record_bytes, size_t scratch_bytes, void **d_tab, void **d_scratch)
{
    void **owned = &ctx->d_batch[which];
    HIP_TRY(hipSetDevice(ctx->device));
    if (!*owned)
        HIP_TRY(hipMalloc(owned, record_bytes * SVT_AMD_MAX_BATCH + scratch_bytes));
    *d_tab = *owned;
    *d_scratch = (uint8_t *)*owned + record_bytes * SVT_AMD_MAX_BATCH;
    if (ctx->num_slots <= (int)sizeof(seen))
        memset(seen, 0, (size_t)ctx->num_slots);
    return SVT_AMD_OK;
}

/* the planes of a slot may have been built on another lane: the launch waits on ev_ready of every slot it reads, once per slot and call */
int svt_amd_batch_wait_slot(SvtAmdContext *ctx, int slot)
{
    uint8_t untracked = 0, *s = ctx->num_slots <= (int)sizeof(seen) ? &seen[slot] : &untracked;
    if (!*s)
        HIP_TRY(hipStreamWaitEvent(svt_amd_ctx_stream(ctx), ctx->slots[slot].ev_ready, 0));
    *s = 1;
    return SVT_AMD_OK;
}

/* the size of a batch that takes it as arguments.  The LCU bound of the entry's kernels is tested first: only a picture within it lets the context be read.
 * must_fit: a picture of more LCUs than the largest the context was made for is refused - per-LCU scratch is sized once, for that one. */
int svt_amd_batch_geometry(const char *entry, const SvtAmdContext *ctx, int luma_width, int luma_height, int max_lcus, bool must_fit, SvtAmdBatchGeometry *g)
{
    const int w = luma_width, h = luma_height, wl = (w + 63) / 64, hl = (h + 63) / 64, lcus = wl * hl;
    if (w < 1 || h < 1 || lcus > max_lcus)
        SVT_AMD_BAD("%s: job 0: a picture of %dx%d (at most %d LCUs)", entry, w, h, max_lcus);
    const int cap_lcus = svt_amd_lcu_count(ctx->max_w, ctx->max_h);
    if (must_fit && lcus > cap_lcus)
        SVT_AMD_BAD("%s: job 0: a picture of %dx%d in a context made for %dx%d", entry, w, h, ctx->max_w, ctx->max_h);
    *g = SvtAmdBatchGeometry{w, h, wl, hl, lcus, (lcus + 3) / 4, cap_lcus, (cap_lcus + 3) / 4};
    return SVT_AMD_OK;
}

/* a job reads the records of `kinds` (BATCH_REC_ME, BATCH_REC_OIS or both) resident in a slot: it has to hold a picture of the batch's size and complete
 * records of it (svt_amd_slot_records) */
int svt_amd_batch_slot_records(const char *entry, SvtAmdContext *ctx, int job, int slot, int kinds, int w, int h)
{
    const DevPicture *c = slot >= 0 && slot < ctx->num_slots ? &ctx->slots[slot] : nullptr;
    if (!c || !c->valid)
        SVT_AMD_BAD("%s: job %d reads the %s records of slot %d, which holds no picture", entry, job, kinds & BATCH_REC_ME ? "ME" : "OIS", slot);
    if (c->width != w || c->height != h)
        SVT_AMD_BAD("%s: job %d: slot %d holds a picture of %dx%d, the batch is %dx%d", entry, job, slot, c->width, c->height, w, h);
    for (int kind = SLOT_ME; kind <= SLOT_OIS; kind++)
        if ((kinds >> kind & 1) && !svt_amd_slot_records(ctx, slot, kind, w, h))
            SVT_AMD_BAD("%s: job %d: slot %d holds no complete %s records", entry, job, slot, kind == SLOT_ME ? "ME" : "OIS");
    return SVT_AMD_OK;
}

/* ... and where its descriptor is filled: the launch waits for the slot's planes (svt_amd_batch_wait_slot) and for the launch that wrote the records, once per
 * distinct producing launch and call (svt_amd_records_wait), and reads *records in place.  kind: SLOT_ME or SLOT_OIS. */
int svt_amd_batch_bind_records(SvtAmdContext *ctx, SvtAmdRecordsBinder *b, int slot, int kind, const void **records)
{
    DevPicture *c = &ctx->slots[slot];
    SVT_AMD_TRY(svt_amd_batch_wait_slot(ctx, slot));
    SVT_AMD_TRY(svt_amd_records_wait(ctx, c, kind, b->waited, &b->nwaited, 32));
    *records = kind == SLOT_ME ? (const void *)c->d_me_out : (const void *)c->d_ois_out;
    return SVT_AMD_OK;
}

/* the next run [*begin, *end) of jobs whose `want` byte (`stride` bytes from one job to the next) is set, from *begin on: one memset clears an output array
 * for a whole run.  for (int i = 0, e; svt_amd_batch_run(&jobs[0].want_x, sizeof(jobs[0]), n, &i, &e); i = e) ... */
bool svt_amd_batch_run(const uint8_t *want, size_t stride, int num_jobs, int *begin, int *end)
{
    int i = *begin;
    while (i < num_jobs && !want[(size_t)i * stride])
        i++;
    int e = i;
    while (e < num_jobs && want[(size_t)e * stride])
        e++;
    *begin = i, *end = e;
    return i < num_jobs;
}

extern "C" size_t svt_amd_side_stats_bytes(uint16_t luma_width, uint16_t luma_height, int which, int regions_w, int regions_h)
{
    const size_t lcus = (size_t)svt_amd_lcu_count(luma_width, luma_height);
    switch (which) {
    case SVT_AMD_SIDE_BLOCK_STATS:
        return lcus * sizeof(SvtAmdPaLcuStats);
    case SVT_AMD_SIDE_AC_ENERGY:
        return lcus * 5 * sizeof(uint64_t);
    case SVT_AMD_SIDE_ZZ:
        return lcus * sizeof(SvtAmdZzLcu);
    case SVT_AMD_SIDE_HISTOGRAM:
        return svt_amd_regions_ok(regions_w, regions_h) ? (size_t)regions_w * regions_h * 256 * sizeof(uint32_t) : 0;
    case SVT_AMD_SIDE_REGION_AVG:
        return 64;
    case SVT_AMD_SIDE_SUM_LUMA:
        return sizeof(uint64_t);
    }
    return 0;
}

extern "C" int svt_amd_side_stats_batch_launch(SvtAmdContext *ctx, const SvtAmdSideJob *jobs, int num_jobs, int regions_w, int regions_h,
                                               const SvtAmdSideArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    int w = 0, h = 0;
    bool any_luma = false, any_hist = false, any_zz = false;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdSideJob &j = jobs[i];
        SVT_AMD_TRY(svt_amd_batch_slot(__func__, ctx, i, j.cur_slot, &w, &h));
        if (j.prev_slot >= 0) {
            if (j.prev_slot >= ctx->num_slots || !ctx->slots[j.prev_slot].valid)
                SVT_AMD_BAD("%s: job %d: previous slot %d holds no picture", __func__, i, j.prev_slot);
            if (ctx->slots[j.prev_slot].width != w || ctx->slots[j.prev_slot].height != h)
                SVT_AMD_BAD("%s: job %d: previous slot %d holds a picture of another size", __func__, i, j.prev_slot);
            if (!out->zz)
                SVT_AMD_BAD("%s: job %d wants the zero-motion SAD, but there is no zz array", __func__, i);
            any_zz = true;
        }
        if (j.want_block_stats && !out->block_stats)
            SVT_AMD_BAD("%s: job %d wants block statistics, but there is no block_stats array", __func__, i);
        if (j.want_ac_energy && !out->ac_energy)
            SVT_AMD_BAD("%s: job %d wants AC energies, but there is no ac_energy array", __func__, i);
        if (j.want_histogram && !out->histogram)
            SVT_AMD_BAD("%s: job %d wants histograms, but there is no histogram array", __func__, i);
        any_luma |= j.want_block_stats || j.want_ac_energy;
        any_hist |= j.want_histogram != 0;
    }
    if (any_hist && (!svt_amd_regions_ok(regions_w, regions_h) || w / 4 < regions_w || h / 4 < regions_h))
        SVT_AMD_BAD("%s: %d x %d regions of a %dx%d picture", __func__, regions_w, regions_h, w, h);
    if (!any_luma && !any_hist && !any_zz)
        return SVT_AMD_OK;
    const int wl = (w + 63) / 64, lcus = svt_amd_lcu_count(w, h), regions = any_hist ? regions_w * regions_h : 0;

    SideJobDev *d_tab;
    unsigned long long *d_sums; /* the per-region sums the histogram kernels accumulate into */
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_SIDE, sizeof(SideJobDev), SIDE_SUMS_BYTES, (void **)&d_tab, (void **)&d_sums));
    const size_t b_stats = (size_t)lcus * sizeof(SvtAmdPaLcuStats), b_hist = (size_t)regions * 256 * 4;
    static thread_local SideJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdSideJob &j = jobs[i];
        const DevPicture *c = &ctx->slots[j.cur_slot], *p = j.prev_slot >= 0 ? &ctx->slots[j.prev_slot] : nullptr;
        SideJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        d.full = j.want_block_stats || j.want_ac_energy ? c->full.origin : nullptr;
        d.six = c->sixteenth.origin;
        d.prev_six = p ? p->sixteenth.origin : nullptr;
        d.pitch_full = c->full.pitch, d.pitch_six = c->sixteenth.pitch;
        d.stats = j.want_block_stats ? (SvtAmdPaLcuStats *)((uint8_t *)out->block_stats + (size_t)i * b_stats) : nullptr;
        d.energy = j.want_ac_energy ? (unsigned long long *)out->ac_energy + (size_t)i * lcus * 5 : nullptr;
        d.zz = p ? out->zz + (size_t)i * lcus : nullptr;
        if (j.want_histogram) {
            d.hist = out->histogram + (size_t)i * regions * 256;
            d.sums = d_sums + (size_t)i * 64;
            d.region_avg = out->region_average ? out->region_average + (size_t)i * 64 : nullptr;
            d.total = out->sum_luma ? (unsigned long long *)out->sum_luma + i : nullptr;
        }
        /* the planes may have been built on another lane: the current AND the previous slot */
        SVT_AMD_TRY(svt_amd_batch_wait_slot(ctx, j.cur_slot));
        if (p)
            SVT_AMD_TRY(svt_amd_batch_wait_slot(ctx, j.prev_slot));
    }
    /* the table goes up in stream order (a copy kernel from a pinned ring): a batch queued behind another one on this lane does not overwrite the
     * table the first one still reads */
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(SideJobDev) * (size_t)num_jobs));
    if (any_hist) { /* what the histogram kernels accumulate into: one memset per run of pictures that want them */
        HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)num_jobs * 64 * 8, st));
        for (int i = 0, e; svt_amd_batch_run(&jobs[0].want_histogram, sizeof(jobs[0]), num_jobs, &i, &e); i = e) {
            HIP_TRY(hipMemsetAsync(out->histogram + (size_t)i * regions * 256, 0, (size_t)(e - i) * b_hist, st));
            if (out->sum_luma)
                HIP_TRY(hipMemsetAsync(out->sum_luma + i, 0, (size_t)(e - i) * 8, st));
        }
    }
    if (any_luma)
        hipLaunchKernelGGL(k_side_luma, dim3((unsigned)lcus, (unsigned)num_jobs), dim3(64), 0, st, (const SideJobDev *)d_tab, w, h, wl);
    if (any_hist) {
        hipLaunchKernelGGL(k_side_hist, dim3(SIDE_STRIPS, (unsigned)regions, (unsigned)num_jobs), dim3(256), 0, st, (const SideJobDev *)d_tab, w / 4, h / 4, regions_w,
                           regions_h);
        hipLaunchKernelGGL(k_side_hist_finish, dim3((unsigned)regions, (unsigned)num_jobs), dim3(256), 0, st, (const SideJobDev *)d_tab, w / 4, h / 4, regions_w, regions_h);
    }
    if (any_zz)
        hipLaunchKernelGGL(k_side_zz, dim3((unsigned)((lcus + 3) / 4), (unsigned)num_jobs), dim3(256), 0, st, (const SideJobDev *)d_tab, w, h, lcus, wl);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
