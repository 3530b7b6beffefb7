/*
 * handoff_kernels.hip - the entropy hand-off pre-scan (include/svt_hevc_amd.h "Entropy hand-off pre-scan"): one device chain behind two
 * kinds of caller.  What EncodeQuantizedCoefficients (Codec/EbEntropyCoding.c:1172) does with a transform block before its first bin, for every transform block of
 * a picture, from the records where they lie in HBM: per block 8 bytes, per coded sub-block 8, per non-zero coefficient 2, packed in LCU order.
 *   svt_amd_entropy_handoff_launch, svt_amd_encdec_picture_entropy_handoff: the last stream-ordered stage of the picture chain, into DEVICE arrays of the caller - no
 *                         synchronisation, no host memory, no working memory of the context.
 *   svt_amd_coeff_scan_picture: the blocking call, into arrays carved from the context's scratch; it uploads host records, waits and downloads.
 * What the kernels pass to one another lies in the output arrays (the per-LCU counts are fields of SvtAmdCoeffScanLcu; the LCU's check status travels in its pad[0]
 * from the count kernel to the base kernel, which reads it and writes the 0 the contract asks for).  The per-LCU digest is coeffscan_device.h.
 *   k_handoff_lcu<false>  count: a 256-thread workgroup per LCU.  Validates the record, builds the block table, reads every coded sub-block (four 8-byte loads,
 *                         the 16 values in registers) for its significance map, and writes the complete SvtAmdCoeffScanLcu - every tu, groups, levels - and
 *                         the optional copies of the record heads.
 *   k_handoff_bases       one workgroup: exclusive sums of the counts over the LCUs in chunks of 1024, as many as there are -> group_base / level_base, the
 *                         totals, the overflow bits and the check sums in `head`.
 *   k_handoff_lcu<true>   write: a workgroup per LCU again; LCUs without a group, or whose lists both do not fit, leave at once.  Reads the sub-blocks a second
 *                         time, digests them (signs, greater-1 flags, levels) and stores group and levels at their picture offsets.
 * No workgroup waits for another one: the order between the three kernels is stream order.  Every store is guarded by n_lcus and by the capacities, every load of a
 * unit or a coefficient by the validity rules (hf_unit_ok and the area rule below), whatever the records hold.
 * Bound: HBM - the s16 planes of the coded blocks are read twice (at most 2 * 3 * W * H bytes at 4:2:0); the output is a few percent of that and is written once,
 * where it belongs.
 */
#include <string.h>
#include "coeffscan_device.h"
#include "encdec_device.h"
#include "pa_batch.h"

#define HF_WORK_HEAD offsetof(SvtAmdLcuWork, src_y)     /* head + unit list: 1584 */
#define HF_RESULT_HEAD offsetof(SvtAmdLcuResult, coeff_y) /* cbf / count records: 768 */
#define HF_RESULT_MIN offsetof(SvtAmdLcuResult, rec_y)    /* ... and the coefficient planes */
#define HF_BAD_LCU 0x80u
static_assert(HF_WORK_HEAD == 1584 && HF_RESULT_HEAD == 768 && HF_RESULT_HEAD == sizeof(SvtAmdLcuCuResult) * SVT_AMD_LCU_MAX_CUS, "record heads");
static_assert(offsetof(SvtAmdLcuWork16, src_y) == HF_WORK_HEAD && offsetof(SvtAmdLcuResult16, coeff_y) == HF_RESULT_HEAD && offsetof(SvtAmdLcuResult16, rec_y) == HF_RESULT_MIN,
              "the 8- and 16-bit records share heads and coefficient planes");
static_assert(sizeof(SvtAmdEntropyHandoffHead) == 32 && sizeof(SvtAmdCoeffScanLcu) == 1552 && sizeof(SvtAmdCoeffScanGroup) == 8, "hand-off records");

struct HandoffArgs {
    const uint8_t *works, *results;
    size_t work_stride, result_stride;
    uint32_t n_lcus, group_capacity, level_capacity;
    SvtAmdEntropyHandoffHead *head;
    SvtAmdCoeffScanLcu *lcus;
    SvtAmdCoeffScanGroup *groups;
    uint16_t *levels;
    uint32_t *work_heads, *result_heads;
};

/* the rules a unit must keep to be scanned (tests/handoff_numpy.py restates them): a size of 8 / 16 / 32 / 64, x and y multiples of 8, inside the LCU, and a 64x64
 * unit the only unit of its LCU (inside the LCU it then lies at (0, 0)).  With them every coefficient of its blocks lies in the LCU's planes, 8 bytes a row of
 * four at a multiple of 8 bytes from the plane's start. */
__device__ __forceinline__ bool hf_unit_ok(const SvtAmdLcuCu &u, int ncu)
{
    const uint32_t x = u.x, y = u.y, s = u.size;
    if (s != 8 && s != 16 && s != 32 && s != 64)
        return false;
    if ((x | y) & 7u)
        return false;
    if (x + s > 64 || y + s > 64)
        return false;
    return s != 64 || ncu == 1;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_handoff_lcu(const HandoffArgs A)
{
    __shared__ CsShared S;
    const int t = threadIdx.x;
    const uint32_t lcu = blockIdx.x;
    if (lcu >= A.n_lcus)
        return;
    uint32_t gb = 0, lb = 0, ng = 0, nl = 0;
    bool fit_g = false, fit_l = false;
    if (WRITE) { /* workgroup-uniform: what the count and the base kernel left */
        gb = A.lcus[lcu].group_base, lb = A.lcus[lcu].level_base, ng = A.lcus[lcu].groups, nl = A.lcus[lcu].levels;
        fit_g = ng <= CS_MAX_SUBS && gb <= A.group_capacity && ng <= A.group_capacity - gb;
        fit_l = nl <= CS_MAX_LEVELS && lb <= A.level_capacity && nl <= A.level_capacity - lb;
        if (!ng || (!fit_g && !fit_l))
            return;
    }
    const SvtAmdLcuWork *W = (const SvtAmdLcuWork *)(A.works + (size_t)lcu * A.work_stride);
    const SvtAmdLcuResult *R = (const SvtAmdLcuResult *)(A.results + (size_t)lcu * A.result_stride);
    /* ---- 0. the record: an LCU is refused when it lists more than 64 units, or when its well-formed units cover more than its 64 x 64 samples (they overlap: the
     * lists of an LCU hold 384 sub-blocks) ---- */
    const int ncu = W->num_cus;
    const bool long_list = ncu > SVT_AMD_LCU_MAX_CUS;
    bool unit_bad = false;
    uint32_t area = 0; /* in 8 x 8 blocks: a wave's sum stays below 2^16 (cs_scan256) */
    if (!long_list && t < ncu) {
        const SvtAmdLcuCu &u = W->cu[t];
        unit_bad = !hf_unit_ok(u, ncu);
        area = unit_bad ? 0u : ((uint32_t)u.size >> 3) * ((uint32_t)u.size >> 3);
    }
    uint32_t covered;
    cs_scan256(S, area, &covered);
    const bool refused = long_list || covered > 64u;
    /* ---- 1. the LCU's transform blocks ---- */
    uint32_t nsub = 0;
    if (t < CS_MAX_TUS) {
        const int c = t / 3, p = t - 3 * c;
        CsTu T = cs_tu_none(p);
        if (!refused) {
            const bool big = ncu == 1 && W->cu[0].size == 64;
            const bool exists = big ? (c >= 1 && c <= 4) : c < ncu;
            if (exists && hf_unit_ok(W->cu[big ? 0 : c], ncu) && R->cu[c].cbf[p])
                nsub = cs_tu_build(T, W->cu[big ? 0 : c], R->cu[c].nz[p], big, c, p);
        }
        S.tu[t] = T;
    }
    const uint32_t total_subs = cs_place_blocks(S, t, nsub); /* <= CS_MAX_SUBS by the area rule: a unit of s x s samples has s * s / 16 + 2 * s * s / 64 sub-blocks */
    /* ---- 2. a thread per sub-block ---- */
    CsSub sub[2];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t q = (uint32_t)t + 256u * pass;
        sub[pass].sig = 0, sub[pass].cnt = 0, sub[pass].sign = 0, sub[pass].gt1 = 0;
        if (q < total_subs && q < CS_MAX_SUBS) {
            int16_t v[16];
            const int scan = cs_load_sub(S, R, q, v);
            if (WRITE)
                cs_digest_scan(scan, v, sub[pass]);
            else
                sub[pass].sig = cs_sigmap(scan, v), sub[pass].cnt = (uint32_t)__popc(sub[pass].sig);
            S.sig[q] = (uint16_t)sub[pass].sig, S.cnt[q] = (uint8_t)sub[pass].cnt;
        }
    }
    __syncthreads();
    /* ---- 3. per block: last sub-block, groups and levels ---- */
    uint32_t total_groups, total_levels;
    const SvtAmdCoeffScanTu o = cs_finish_blocks(S, t, &total_groups, &total_levels);
    if (!WRITE) {
        SvtAmdCoeffScanLcu *out = A.lcus + lcu;
        if (t < CS_MAX_TUS)
            out->tu[t % 3][t / 3] = o;
        const uint32_t bad_units = (uint32_t)__syncthreads_count(unit_bad);
        if (t == 0) {
            out->group_base = 0, out->level_base = 0;
            out->groups = (uint16_t)total_groups, out->levels = (uint16_t)total_levels;
            out->pad[0] = (uint8_t)(refused ? HF_BAD_LCU : bad_units), out->pad[1] = out->pad[2] = out->pad[3] = 0; /* pad[0]: for k_handoff_bases, which zeroes it */
        }
        /* the heads as they are, refused LCUs too: a copy, not a judgement */
        if (A.work_heads)
            for (uint32_t i = t; i < HF_WORK_HEAD / 4; i += 256)
                A.work_heads[(size_t)lcu * (HF_WORK_HEAD / 4) + i] = ((const uint32_t *)W)[i];
        if (A.result_heads && t < HF_RESULT_HEAD / 4)
            A.result_heads[(size_t)lcu * (HF_RESULT_HEAD / 4) + t] = ((const uint32_t *)R)[t];
        return;
    }
    __syncthreads();
    /* ---- 4. the sub-block threads store their group and levels at the picture offsets, each list where the LCU's whole range fits ---- */
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t q = (uint32_t)t + 256u * pass;
        if (q < total_subs && q < CS_MAX_SUBS && S.grp[q] >= 0) {
            const uint32_t g_at = (uint32_t)S.grp[q], l_at = S.lvl_off[q];
            if (fit_g && g_at < ng) {
                SvtAmdCoeffScanGroup g;
                g.sigmap = (uint16_t)sub[pass].sig, g.sign = (uint16_t)sub[pass].sign, g.gt1 = (uint16_t)sub[pass].gt1, g.first_level = (uint16_t)l_at;
                A.groups[gb + g_at] = g;
            }
            if (fit_l) {
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if ((uint32_t)i < sub[pass].cnt && l_at + i < nl)
                        A.levels[lb + l_at + i] = sub[pass].level[i];
            }
        }
    }
}

/* picture offsets of the LCUs' lists, the totals and the check sums: one workgroup, LCUs in chunks of 1024 */
__global__ __launch_bounds__(1024) void k_handoff_bases(const HandoffArgs A)
{
    __shared__ uint32_t wt[2][16];
    __shared__ uint32_t carry[2];
    __shared__ uint32_t chk[4][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = (int)A.n_lcus;
    if (t < 2)
        carry[t] = 0;
    __syncthreads();
    uint32_t bad_lcus = 0, first_bad_lcu = 0xFFFFFFFFu, bad_units = 0, first_bad_unit_lcu = 0xFFFFFFFFu;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        uint32_t v[2] = {i < n ? A.lcus[i].groups : 0u, i < n ? A.lcus[i].levels : 0u}, x[2] = {v[0], v[1]};
        if (i < n) {
            const uint32_t status = A.lcus[i].pad[0];
            if (status & HF_BAD_LCU)
                bad_lcus++, first_bad_lcu = min(first_bad_lcu, (uint32_t)i);
            else if (status)
                bad_units += status, first_bad_unit_lcu = min(first_bad_unit_lcu, (uint32_t)i);
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x[k], d);
                if (lane >= d)
                    x[k] += y;
            }
            if (lane == 63)
                wt[k][wave] = x[k];
        }
        __syncthreads();
        uint32_t pre[2] = {carry[0], carry[1]}, sum[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 2; k++)
            for (int w = 0; w < 16; w++) {
                if (w < wave)
                    pre[k] += wt[k][w];
                sum[k] += wt[k][w];
            }
        if (i < n) {
            A.lcus[i].group_base = pre[0] + x[0] - v[0], A.lcus[i].level_base = pre[1] + x[1] - v[1];
            A.lcus[i].pad[0] = 0;
        }
        __syncthreads();
        if (t < 2)
            carry[t] += sum[t];
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) {
        bad_lcus += (uint32_t)__shfl_xor((int)bad_lcus, o), bad_units += (uint32_t)__shfl_xor((int)bad_units, o);
        first_bad_lcu = min(first_bad_lcu, (uint32_t)__shfl_xor((int)first_bad_lcu, o));
        first_bad_unit_lcu = min(first_bad_unit_lcu, (uint32_t)__shfl_xor((int)first_bad_unit_lcu, o));
    }
    if (lane == 0)
        chk[0][wave] = bad_lcus, chk[1][wave] = first_bad_lcu, chk[2][wave] = bad_units, chk[3][wave] = first_bad_unit_lcu;
    __syncthreads();
    if (t == 0) {
        SvtAmdEntropyHandoffHead h;
        h.groups = carry[0], h.levels = carry[1];
        h.overflow = (carry[0] > A.group_capacity ? 1u : 0u) | (carry[1] > A.level_capacity ? 2u : 0u);
        h.bad_lcus = 0, h.first_bad_lcu = 0xFFFFFFFFu, h.bad_units = 0, h.first_bad_unit_lcu = 0xFFFFFFFFu, h.pad = 0;
        for (int w = 0; w < 16; w++) {
            h.bad_lcus += chk[0][w], h.bad_units += chk[2][w];
            h.first_bad_lcu = min(h.first_bad_lcu, chk[1][w]), h.first_bad_unit_lcu = min(h.first_bad_unit_lcu, chk[3][w]);
        }
        *A.head = h;
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

extern "C" size_t svt_amd_entropy_handoff_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    if (luma_width < 1 || luma_height < 1)
        return 0;
    const size_t n = (size_t)svt_amd_lcu_count(luma_width, luma_height);
    switch (which) {
    case SVT_AMD_ENTROPY_HANDOFF_HEAD: return sizeof(SvtAmdEntropyHandoffHead);
    case SVT_AMD_ENTROPY_HANDOFF_LCUS: return n * sizeof(SvtAmdCoeffScanLcu);
    case SVT_AMD_ENTROPY_HANDOFF_GROUPS: return n * CS_MAX_SUBS * sizeof(SvtAmdCoeffScanGroup);
    case SVT_AMD_ENTROPY_HANDOFF_LEVELS: return n * CS_MAX_LEVELS * sizeof(uint16_t);
    case SVT_AMD_ENTROPY_HANDOFF_WORK_HEADS: return n * HF_WORK_HEAD;
    case SVT_AMD_ENTROPY_HANDOFF_RESULT_HEADS: return n * HF_RESULT_HEAD;
    default: return 0;
    }
}

/* everything the host can judge of the output arrays; `entry`: the public entry that was called */
static int handoff_out_ok(const char *entry, const SvtAmdEntropyHandoffOut *out)
{
    if (!out || !out->head || !out->lcus || !out->groups || !out->levels)
        SVT_AMD_BAD("%s: device arrays for head, lcus, groups and levels", entry);
    if ((uintptr_t)out->head % 4 || (uintptr_t)out->lcus % 4 || (uintptr_t)out->groups % 8 || (uintptr_t)out->levels % 2 || (uintptr_t)out->work_heads % 4 ||
        (uintptr_t)out->result_heads % 4)
        SVT_AMD_BAD("%s: head at %p, lcus at %p, the head copies at %p / %p (4-byte aligned), groups at %p (8-byte aligned) or levels at %p (2-byte aligned)", entry,
                    (void *)out->head, (void *)out->lcus, out->work_heads, (void *)out->result_heads, (void *)out->groups, (void *)out->levels);
    return SVT_AMD_OK;
}

/* the one device chain of the hand-off: the scan tables once a device, then the three kernels on the context's stream.  What a caller has to check of its
 * parameters it has checked, and the device is the context's. */
static int handoff_run(SvtAmdContext *ctx, const HandoffArgs &A)
{
    SVT_AMD_TRY(rate_tables_once(ctx->device));
    hipStream_t st = svt_amd_ctx_stream(ctx);
    hipLaunchKernelGGL(k_handoff_lcu<false>, dim3(A.n_lcus), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_handoff_bases, dim3(1), dim3(1024), 0, st, A);
    hipLaunchKernelGGL(k_handoff_lcu<true>, dim3(A.n_lcus), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

static int handoff_queue(const char *entry, SvtAmdContext *ctx, const SvtAmdEntropyHandoffJob *job, const SvtAmdEntropyHandoffOut *out)
{
    /* ---- everything is checked before anything is queued ---- */
    if (!job->d_works || !job->d_results)
        SVT_AMD_BAD("%s: the job has no work or no result records", entry);
    if (job->work_stride < HF_WORK_HEAD || job->work_stride % 4 || (uintptr_t)job->d_works % 4)
        SVT_AMD_BAD("%s: work records %zu bytes apart at %p (words; at least the %zu bytes of head and unit list)", entry, job->work_stride, job->d_works, (size_t)HF_WORK_HEAD);
    if (job->result_stride < HF_RESULT_MIN || job->result_stride % 4 || (uintptr_t)job->d_results % 4)
        SVT_AMD_BAD("%s: result records %zu bytes apart at %p (words; at least the %zu bytes in front of the reconstruction)", entry, job->result_stride, job->d_results,
                    (size_t)HF_RESULT_MIN);
    if (job->n_lcus < 1 || job->n_lcus > SVT_AMD_MDCTL_MAX_LCUS)
        SVT_AMD_BAD("%s: %u LCUs (1 to %d)", entry, job->n_lcus, SVT_AMD_MDCTL_MAX_LCUS);
    if (job->pad)
        SVT_AMD_BAD("%s: the job's pad is not 0", entry);
    SVT_AMD_TRY(handoff_out_ok(entry, out));

    HIP_TRY(hipSetDevice(ctx->device));
    HandoffArgs A;
    A.works = (const uint8_t *)job->d_works, A.results = (const uint8_t *)job->d_results, A.work_stride = job->work_stride, A.result_stride = job->result_stride;
    A.n_lcus = job->n_lcus, A.group_capacity = job->group_capacity, A.level_capacity = job->level_capacity;
    A.head = out->head, A.lcus = out->lcus, A.groups = out->groups, A.levels = out->levels;
    A.work_heads = (uint32_t *)out->work_heads, A.result_heads = (uint32_t *)out->result_heads;
    return handoff_run(ctx, A);
}

extern "C" int svt_amd_entropy_handoff_launch(SvtAmdContext *ctx, const SvtAmdEntropyHandoffJob *job, const SvtAmdEntropyHandoffOut *out)
{
    if (!ctx || !job || !out)
        SVT_AMD_BAD("%s: a context, a job and the output arrays", __func__);
    return handoff_queue(__func__, ctx, job, out);
}

/* the same on the records the last mode-decision call on `pic` - blocking or launched - left in HBM */
extern "C" int svt_amd_encdec_picture_entropy_handoff(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, uint32_t group_capacity, uint32_t level_capacity,
                                                      const SvtAmdEntropyHandoffOut *out)
{
    if (!ctx || !pic || !out)
        SVT_AMD_BAD("%s: a context, a picture object and the output arrays", __func__);
    SVT_AMD_TRY(handoff_out_ok(__func__, out));
    if (pic->device != ctx->device)
        SVT_AMD_BAD("%s: the picture object lives on device %d, the context on device %d", __func__, pic->device, ctx->device);
    if (pic->md_rect_n)
        SVT_AMD_BAD("%s: the picture object has a rank rectangle (svt_amd_encdec_picture_set_rect): the records of its other LCUs are zeroed", __func__);
    SvtAmdEntropyHandoffJob job;
    memset(&job, 0, sizeof(job));
    if (!pic->md_works_whole || !svt_amd_md_picture_records(pic, &job.d_works, &job.work_stride, &job.d_results, &job.result_stride))
        SVT_AMD_BAD("%s: no svt_amd_md_encode_picture* call that writes work records has completed on the picture object", __func__);
    job.n_lcus = (uint32_t)pic->nlcu, job.group_capacity = group_capacity, job.level_capacity = level_capacity;
    return handoff_queue(__func__, ctx, &job, out);
}

/* The blocking entry: the same chain into arrays carved from the context's scratch, and what is this entry's own - its parameter checks, the upload of host
 * records, the downloads, the two waits and the return codes. */
extern "C" int svt_amd_coeff_scan_picture(SvtAmdContext *ctx, const void *works, size_t work_stride, const void *results, size_t result_stride,
                                          int device_arrays, int n_lcus, SvtAmdCoeffScanLcu *lcus, SvtAmdCoeffScanGroup *groups, uint32_t group_capacity,
                                          uint16_t *levels, uint32_t level_capacity, uint32_t totals[2])
{
    if (!ctx || !works || !results || !lcus || !groups || !levels || !totals || n_lcus < 1 || work_stride < HF_WORK_HEAD || result_stride < HF_RESULT_MIN) {
        svt_amd_set_error("svt_amd_coeff_scan_picture: bad parameter");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (device_arrays && ((uintptr_t)works % 4 || (uintptr_t)results % 4 || work_stride % 4 || result_stride % 4)) /* the kernels read the records in place, by words */
        SVT_AMD_BAD("%s: device records at %p / %p, %zu / %zu bytes apart (4-byte aligned, strides multiples of 4)", __func__, works, results, work_stride, result_stride);
    HIP_TRY(hipSetDevice(ctx->device));
    const auto up256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t n = (size_t)n_lcus;
    /* a capacity above the worst case can never overflow: the scratch holds no more than that */
    const size_t gcap = group_capacity < n * CS_MAX_SUBS ? group_capacity : n * CS_MAX_SUBS, lcap = level_capacity < n * CS_MAX_LEVELS ? level_capacity : n * CS_MAX_LEVELS;
    const size_t b_lcus = up256(n * sizeof(SvtAmdCoeffScanLcu)), b_groups = up256(gcap * sizeof(SvtAmdCoeffScanGroup)), b_levels = up256(lcap * sizeof(uint16_t));
    const size_t b_works = device_arrays ? 0 : up256(n * HF_WORK_HEAD), b_results = device_arrays ? 0 : up256(n * HF_RESULT_MIN);
    uint8_t *d = nullptr;
    SVT_AMD_TRY(svt_amd_ctx_scratch(ctx, 256 + b_lcus + b_groups + b_levels + b_works + b_results, &d));
    hipStream_t st = svt_amd_ctx_stream(ctx);
    HandoffArgs A;
    A.works = (const uint8_t *)works, A.results = (const uint8_t *)results, A.work_stride = work_stride, A.result_stride = result_stride;
    A.n_lcus = (uint32_t)n_lcus, A.group_capacity = (uint32_t)gcap, A.level_capacity = (uint32_t)lcap;
    A.head = (SvtAmdEntropyHandoffHead *)d, A.lcus = (SvtAmdCoeffScanLcu *)(d + 256);
    A.groups = (SvtAmdCoeffScanGroup *)((uint8_t *)A.lcus + b_lcus), A.levels = (uint16_t *)((uint8_t *)A.groups + b_groups);
    A.work_heads = nullptr, A.result_heads = nullptr;
    if (!device_arrays) { /* only the heads travel: unit lists without the source samples, flags + coefficients without the reconstruction */
        uint8_t *dw = (uint8_t *)A.levels + b_levels, *dr = dw + b_works;
        HIP_TRY(hipMemcpy2DAsync(dw, HF_WORK_HEAD, works, work_stride, HF_WORK_HEAD, n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(dr, HF_RESULT_MIN, results, result_stride, HF_RESULT_MIN, n, hipMemcpyHostToDevice, st));
        A.works = dw, A.results = dr, A.work_stride = HF_WORK_HEAD, A.result_stride = HF_RESULT_MIN;
    }
    SVT_AMD_TRY(handoff_run(ctx, A));
    SvtAmdEntropyHandoffHead head;
    HIP_TRY(hipMemcpyAsync(&head, A.head, sizeof(head), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lcus, A.lcus, n * sizeof(SvtAmdCoeffScanLcu), hipMemcpyDeviceToHost, st));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    totals[0] = head.groups, totals[1] = head.levels;
    if (head.bad_lcus || head.bad_units) /* lcus[] says which: a refused LCU or unit reads "nothing to code" */
        SVT_AMD_BAD("%s: malformed records: %u bad LCUs (first %d), %u bad units (first in LCU %d); no list is returned", __func__, head.bad_lcus, (int)head.first_bad_lcu,
                    head.bad_units, (int)head.first_bad_unit_lcu);
    if (head.overflow) {
        svt_amd_set_error("svt_amd_coeff_scan_picture: %u groups / %u levels do not fit the capacities %u / %u", totals[0], totals[1], group_capacity, level_capacity);
        return SVT_AMD_ERR_RESOURCES;
    }
    if (totals[0])
        HIP_TRY(hipMemcpyAsync(groups, A.groups, (size_t)totals[0] * sizeof(SvtAmdCoeffScanGroup), hipMemcpyDeviceToHost, st));
    if (totals[1])
        HIP_TRY(hipMemcpyAsync(levels, A.levels, (size_t)totals[1] * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    return SVT_AMD_OK;
}
