/*
 * coeffscan_kernels.hip - entropy hand-off pre-scan (include/svt_hevc_amd.h "Entropy hand-off pre-scan").
 *
 * What EncodeQuantizedCoefficients (Codec/EbEntropyCoding.c:1172) does with a transform block before its first bin - mode-dependent scan
 * :1347-1372, sub-block / scan re-ordering with one significance map per 4x4 sub-block :1378-1430, last significant position :1432-1461, the
 * DC-only fast track :1308 - and the sign / greater-1 words its level loop derives from the same values (:1532-1600), for EVERY transform block of
 * a picture in one launch, from the encode pass's records where they lie in HBM.  The host's CABAC loop (integration/svt_coeff_scan_consumer.h) then
 * reads 8 bytes per block, 8 per coded sub-block and 2 per non-zero coefficient instead of the s16 planes.
 *
 * k_coeff_scan: one 256-thread workgroup per LCU.  A THREAD owns a 4x4 sub-block (an LCU has at most 384 of them over its three planes: two
 * passes): four 8-byte loads, the 16 values stay in registers; significance map, count, sign and greater-1 words are bit operations on them.
 * What needs the whole block (last sub-block, where its groups and levels start) is three small exclusive scans over the LCU's <= 192 blocks
 * in LDS.  Groups and levels go to per-LCU pools; k_coeff_scan_bases (one workgroup) turns the per-LCU counts into picture offsets and
 * k_coeff_scan_compact packs the pools in LCU order, so the host copies exactly what was produced.
 * Bound: HBM - the s16 planes are read once (3 * W * H bytes at 4:2:0), the output is a few percent of that.
 * The per-LCU digest - block table, workgroup scan, scans, the digest of a sub-block, the per-block lists - is coeffscan_device.h, which the stream-ordered
 * launch (handoff_kernels.hip) compiles as well.
 */
#include "coeffscan_device.h"

__global__ __launch_bounds__(256) void k_coeff_scan(const uint8_t *__restrict__ works, size_t work_stride, const uint8_t *__restrict__ results,
                                                    size_t result_stride, SvtAmdCoeffScanLcu *__restrict__ lcus,
                                                    SvtAmdCoeffScanGroup *__restrict__ group_pool, uint16_t *__restrict__ level_pool)
{
    __shared__ CsShared S;
    const int t = threadIdx.x, lcu = blockIdx.x;
    const SvtAmdLcuWork *W = (const SvtAmdLcuWork *)(works + (size_t)lcu * work_stride);
    const SvtAmdLcuResult *R = (const SvtAmdLcuResult *)(results + (size_t)lcu * result_stride);
    /* ---- 1. the LCU's transform blocks: block i = 3 * slot + plane ---- */
    uint32_t nsub = 0;
    if (t < CS_MAX_TUS) {
        const int c = t / 3, p = t - 3 * c;
        const int ncu = W->num_cus;
        const bool big = ncu == 1 && W->cu[0].size == 64;
        CsTu T = cs_tu_none(p);
        const bool exists = big ? (c >= 1 && c <= 4) : c < ncu;
        if (exists && R->cu[c].cbf[p])
            nsub = cs_tu_build(T, W->cu[big ? 0 : c], R->cu[c].nz[p], big, c, p);
        S.tu[t] = T;
    }
    const uint32_t total_subs = cs_place_blocks(S, t, nsub);
    /* ---- 2. a thread per sub-block: values into registers, maps / counts into LDS ---- */
    CsSub sub[2];
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t q = (uint32_t)t + 256u * pass;
        sub[pass].sig = 0, sub[pass].cnt = 0, sub[pass].sign = 0, sub[pass].gt1 = 0;
        if (q < total_subs) {
            int16_t v[16];
            const int scan = cs_load_sub(S, R, q, v);
            cs_digest_scan(scan, v, sub[pass]);
            S.sig[q] = (uint16_t)sub[pass].sig, S.cnt[q] = (uint8_t)sub[pass].cnt;
        }
    }
    __syncthreads();
    /* ---- 3. per block: last sub-block, number of groups and levels ---- */
    uint32_t total_groups, total_levels;
    const SvtAmdCoeffScanTu o = cs_finish_blocks(S, t, &total_groups, &total_levels);
    if (t < CS_MAX_TUS)
        lcus[lcu].tu[t % 3][t / 3] = o;
    if (t == 0) {
        lcus[lcu].group_base = 0, lcus[lcu].level_base = 0;
        lcus[lcu].groups = (uint16_t)total_groups, lcus[lcu].levels = (uint16_t)total_levels;
        lcus[lcu].pad[0] = lcus[lcu].pad[1] = lcus[lcu].pad[2] = lcus[lcu].pad[3] = 0;
    }
    __syncthreads();
    /* ---- 4. the sub-block threads write their group and levels into the LCU's pools ---- */
    SvtAmdCoeffScanGroup *gp = group_pool + (size_t)lcu * CS_MAX_SUBS;
    uint16_t *lp = level_pool + (size_t)lcu * CS_MAX_LEVELS;
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t q = (uint32_t)t + 256u * pass;
        if (q < total_subs && S.grp[q] >= 0) {
            SvtAmdCoeffScanGroup g;
            g.sigmap = (uint16_t)sub[pass].sig, g.sign = (uint16_t)sub[pass].sign, g.gt1 = (uint16_t)sub[pass].gt1, g.first_level = S.lvl_off[q];
            gp[S.grp[q]] = g;
#pragma unroll
            for (int i = 0; i < 16; i++)
                if ((uint32_t)i < sub[pass].cnt)
                    lp[S.lvl_off[q] + i] = sub[pass].level[i];
        }
    }
}

/* picture offsets of the LCUs' lists: one workgroup, LCUs in chunks of 1024 */
__global__ __launch_bounds__(1024) void k_coeff_scan_bases(SvtAmdCoeffScanLcu *lcus, int n, uint32_t *totals)
{
    __shared__ uint32_t wt[2][16];
    __shared__ uint32_t carry[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < 2)
        carry[t] = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        uint32_t v[2] = {i < n ? lcus[i].groups : 0u, i < n ? lcus[i].levels : 0u}, x[2] = {v[0], v[1]};
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
        if (i < n)
            lcus[i].group_base = pre[0] + x[0] - v[0], lcus[i].level_base = pre[1] + x[1] - v[1];
        __syncthreads();
        if (t < 2)
            carry[t] += sum[t];
        __syncthreads();
    }
    if (t < 2)
        totals[t] = carry[t];
}

__global__ __launch_bounds__(256) void k_coeff_scan_compact(const SvtAmdCoeffScanLcu *__restrict__ lcus, const SvtAmdCoeffScanGroup *__restrict__ group_pool,
                                                            const uint16_t *__restrict__ level_pool, SvtAmdCoeffScanGroup *__restrict__ groups,
                                                            uint32_t group_capacity, uint16_t *__restrict__ levels, uint32_t level_capacity)
{
    const int lcu = blockIdx.x;
    const uint32_t gb = lcus[lcu].group_base, lb = lcus[lcu].level_base, ng = lcus[lcu].groups, nl = lcus[lcu].levels;
    if (gb + ng <= group_capacity)
        for (uint32_t i = threadIdx.x; i < ng; i += 256)
            groups[gb + i] = group_pool[(size_t)lcu * CS_MAX_SUBS + i];
    if (lb + nl <= level_capacity)
        for (uint32_t i = threadIdx.x; i < nl; i += 256)
            levels[lb + i] = level_pool[(size_t)lcu * CS_MAX_LEVELS + i];
}

extern "C" int svt_amd_coeff_scan_picture(SvtAmdContext *ctx, const void *works, size_t work_stride, const void *results, size_t result_stride,
                                          int device_arrays, int n_lcus, SvtAmdCoeffScanLcu *lcus, SvtAmdCoeffScanGroup *groups, uint32_t group_capacity,
                                          uint16_t *levels, uint32_t level_capacity, uint32_t totals[2])
{
    const size_t work_head = offsetof(SvtAmdLcuWork, src_y), result_head = offsetof(SvtAmdLcuResult, rec_y);
    static_assert(offsetof(SvtAmdLcuWork16, src_y) == offsetof(SvtAmdLcuWork, src_y) && offsetof(SvtAmdLcuResult16, rec_y) == offsetof(SvtAmdLcuResult, rec_y),
                  "the 8- and 16-bit records share their heads");
    if (!ctx || !works || !results || !lcus || !groups || !levels || !totals || n_lcus < 1 || work_stride < work_head || result_stride < result_head) {
        svt_amd_set_error("svt_amd_coeff_scan_picture: bad parameter");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = rate_tables_once(ctx->device);
    if (rc)
        return rc;
    const size_t n = (size_t)n_lcus;
    const size_t b_lcus = (n * sizeof(SvtAmdCoeffScanLcu) + 255) & ~(size_t)255, b_gpool = n * CS_MAX_SUBS * sizeof(SvtAmdCoeffScanGroup),
                 b_lpool = n * CS_MAX_LEVELS * sizeof(uint16_t);
    const size_t b_works = device_arrays ? 0 : ((n * work_head + 255) & ~(size_t)255), b_results = device_arrays ? 0 : ((n * result_head + 255) & ~(size_t)255);
    uint8_t *d = nullptr;
    rc = svt_amd_ctx_scratch(ctx, 256 + b_lcus + 2 * (b_gpool + b_lpool) + b_works + b_results, &d);
    if (rc)
        return rc;
    uint32_t *d_totals = (uint32_t *)d;
    SvtAmdCoeffScanLcu *d_lcus = (SvtAmdCoeffScanLcu *)(d + 256);
    SvtAmdCoeffScanGroup *d_gpool = (SvtAmdCoeffScanGroup *)(d + 256 + b_lcus), *d_groups = (SvtAmdCoeffScanGroup *)((uint8_t *)d_gpool + b_gpool);
    uint16_t *d_lpool = (uint16_t *)((uint8_t *)d_groups + b_gpool), *d_levels = (uint16_t *)((uint8_t *)d_lpool + b_lpool);
    const uint8_t *d_works = (const uint8_t *)works, *d_results = (const uint8_t *)results;
    if (!device_arrays) { /* only the heads travel: unit lists without the source samples, flags + coefficients without the reconstruction */
        uint8_t *dw = (uint8_t *)d_levels + b_lpool, *dr = dw + b_works;
        HIP_TRY(hipMemcpy2DAsync(dw, work_head, works, work_stride, work_head, n, hipMemcpyHostToDevice, svt_amd_ctx_stream(ctx)));
        HIP_TRY(hipMemcpy2DAsync(dr, result_head, results, result_stride, result_head, n, hipMemcpyHostToDevice, svt_amd_ctx_stream(ctx)));
        d_works = dw, d_results = dr, work_stride = work_head, result_stride = result_head;
    }
    hipLaunchKernelGGL(k_coeff_scan, dim3((unsigned)n_lcus), dim3(256), 0, svt_amd_ctx_stream(ctx), d_works, work_stride, d_results, result_stride, d_lcus, d_gpool, d_lpool);
    hipLaunchKernelGGL(k_coeff_scan_bases, dim3(1), dim3(1024), 0, svt_amd_ctx_stream(ctx), d_lcus, n_lcus, d_totals);
    hipLaunchKernelGGL(k_coeff_scan_compact, dim3((unsigned)n_lcus), dim3(256), 0, svt_amd_ctx_stream(ctx), d_lcus, d_gpool, d_lpool, d_groups, group_capacity, d_levels,
                       level_capacity);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(totals, d_totals, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, svt_amd_ctx_stream(ctx)));
    HIP_TRY(hipMemcpyAsync(lcus, d_lcus, n * sizeof(SvtAmdCoeffScanLcu), hipMemcpyDeviceToHost, svt_amd_ctx_stream(ctx)));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    if (totals[0] > group_capacity || totals[1] > level_capacity) {
        svt_amd_set_error("svt_amd_coeff_scan_picture: %u groups / %u levels do not fit the capacities %u / %u", totals[0], totals[1], group_capacity, level_capacity);
        return SVT_AMD_ERR_RESOURCES;
    }
    if (totals[0])
        HIP_TRY(hipMemcpyAsync(groups, d_groups, (size_t)totals[0] * sizeof(SvtAmdCoeffScanGroup), hipMemcpyDeviceToHost, svt_amd_ctx_stream(ctx)));
    if (totals[1])
        HIP_TRY(hipMemcpyAsync(levels, d_levels, (size_t)totals[1] * sizeof(uint16_t), hipMemcpyDeviceToHost, svt_amd_ctx_stream(ctx)));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    return SVT_AMD_OK;
}
