/*
 * noise_kernels.hip - the noise detection of PicturePreProcessingOperations (Codec/EbPictureAnalysisProcess.c:3338) in the batched, stream-ordered shape of
 * side_kernels.hip / detect_kernels.hip (include/svt_hevc_amd.h "Batched noise detection"): the picture is a grid dimension, the per-picture pointers come from
 * a descriptor table in device memory, nothing is copied to the host.  enableDenoiseSrcFlag is never set (Codec/EbResourceCoordinationProcess.c:304), so what the
 * stage leaves behind is lcuFlatNoiseArray and picNoiseClass; no noise or denoised plane is materialised here.
 *   k_noise_blocks        DetectInputPictureNoise (:2539), QuarterSampleDetectNoise (:2909), SubSampleDetectNoise (:3052): grid (64x64 blocks / 4, pictures), one
 *                         wave per 64x64 block of the plane the picture's method reads (input luma, 1/4 or 1/16 picture), a lane per 8x8 block.  A lane reads its
 *                         ten rows once (8-byte loads, the two side columns as bytes), filters four samples a word (the weak luma filter of getFilteredTypes, :956,
 *                         in 16-bit fields), sums by v_sad_u8 and squares by v_dot4_u32_u8; the mean tree of ComputeVariance16x16 / 32x32 / 64x64 (:377, :231,
 *                         :431) goes up by lane shuffles as far as the method's block size.  The reference's noise picture is one 64-row strip (:2573, :2983,
 *                         :3127): in the decimated methods every block takes the noise variance of the block in the TOP rows of its 64x64 block (one shuffle from
 *                         lane & 7), its denoised variance from its own rows.  The `block64x64Y + 64 > width` branch (:2956, :3100) filters a strip again with the
 *                         C routine; both routines give the same samples wherever a variance is read, so there is nothing to restate.  The noiseBlkVar >> 16
 *                         terms of a workgroup go by one vector atomic into one of eight per-picture partial sums (integer adds: order-free).
 *   k_noise_finish        grid (pictures): totLcuCount is geometry (every block inside the floor(w / 64) x floor(h / 64) 64x64 blocks is evaluated), the class
 *                         ladder of the method, the picture record.
 * Traffic: the plane is read once (1 B/pel of it: 1, 1/4 or 1/16 B per luma sample), one byte per evaluated LCU written.  Measured at a third of the copy rate for the
 * full method: bound by load instructions (10 8-byte and 16 byte loads a lane, eight half lines a wave load) and latency, not by HBM.
 */
#include "pa_batch.h"
#include <string.h>

struct NoiseJobDev {
    const uint8_t *plane;          /* sample (0,0) of the plane the method reads */
    uint8_t *flat;                 /* [lcus rounded up to 64], zeroed by the call */
    SvtAmdNoisePic *pic;
    unsigned long long *red;       /* [NOISE_PARTS] context-owned scratch, zeroed by the call */
    int32_t pitch, w, h;           /* of that plane */
    int32_t level;                 /* the block a variance is taken of: 1 = 16x16 (half), 2 = 32x32 (quarter), 3 = 64x64 (full) */
    uint32_t noise_th;             /* NOISE_MIN_LEVEL_0 / _1 (:33-36) */
    int32_t method;
    int32_t pad[2];
};
static_assert(sizeof(NoiseJobDev) == 64, "NoiseJobDev layout");
#define NOISE_PARTS 8
#define NOISE_RED_BYTES ((size_t)SVT_AMD_MAX_BATCH * NOISE_PARTS * 8)

/* (top + bottom + left + right + 4 * centre) >> 3 of four samples: even and odd bytes in 16-bit fields (8 * 255 fits), no carry between fields */
__device__ __forceinline__ uint32_t noise_filter4(uint32_t t, uint32_t b, uint32_t l, uint32_t r, uint32_t c)
{
    const uint32_t M = 0x00FF00FFu;
    const uint32_t e = (t & M) + (b & M) + (l & M) + (r & M) + ((c & M) << 2);
    const uint32_t o = ((t >> 8) & M) + ((b >> 8) & M) + ((l >> 8) & M) + ((r >> 8) & M) + (((c >> 8) & M) << 2);
    return ((e >> 3) & M) | (((o >> 3) & M) << 8);
}

/* max(c - d, 0) of four samples (CLIP3EQ(0, 255, in - denoised), :1306): 256 + c - d per field, bit 8 says c >= d */
__device__ __forceinline__ uint32_t noise_sub4(uint32_t c, uint32_t d)
{
    const uint32_t M = 0x00FF00FFu;
    const uint32_t e = ((c & M) | 0x01000100u) - (d & M), o = (((c >> 8) & M) | 0x01000100u) - ((d >> 8) & M);
    return (e & (((e >> 8) & 0x00010001u) * 0xFFu)) | ((o & (((o >> 8) & 0x00010001u) * 0xFFu)) << 8);
}

/* grid (ceil(blocks / 4), pictures); lcus_w: LCUs a row of the input picture */
__global__ __launch_bounds__(256) void k_noise_blocks(const NoiseJobDev *__restrict__ jobs, int lcus_w)
{
    __shared__ unsigned long long s_term[4];
    const NoiseJobDev &J = jobs[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w = J.w, h = J.h, bw = w >> 6, nblk = bw * (h >> 6), level = J.level;
    const int blk = (int)blockIdx.x * 4 + wave;
    unsigned long long term = 0;
    if (blk < nblk) { /* wave-uniform */
        const int bx = lane & 7, by = lane >> 3, bx64 = blk % bw, by64 = blk / bw;
        const int X = bx64 * 64 + bx * 8, Y = by64 * 64 + by * 8;
        const ptrdiff_t pitch = J.pitch;
        const uint8_t *p = J.plane + (ptrdiff_t)Y * pitch + X; /* 8-byte aligned: the origin is 128-byte aligned, the pitch a multiple of 256 */
        /* rows Y - 1 and Y + 8, columns X - 1 and X + 8 exist in the plane's padding; what is read there never reaches a filtered sample */
        uint2 prev = *(const uint2 *)(p - pitch), cur = *(const uint2 *)p;
        uint32_t sum_d = 0, sq_d = 0, sum_n = 0, sq_n = 0; /* of the rows a variance reads: all eight, or rows 0, 2, 4, 6 for the 64x64 block (below) */
        const bool all_rows = level != 3;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint8_t *row = p + r * pitch;
            const uint2 next = *(const uint2 *)(row + pitch);
            const uint32_t lf = row[-1], rt = row[8];
            uint32_t d0 = noise_filter4(prev.x, next.x, (cur.x << 8) | lf, (cur.x >> 8) | (cur.y << 24), cur.x);
            uint32_t d1 = noise_filter4(prev.y, next.y, (cur.y << 8) | (cur.x >> 24), (cur.y >> 8) | (rt << 24), cur.y);
            /* the first and last row and column of the plane are copied (:1303-1312); their noise, centre - centre, is 0 by itself */
            const int y = Y + r;
            if (y == 0 || y == h - 1) {
                d0 = cur.x, d1 = cur.y;
            } else {
                if (X == 0)
                    d0 = (d0 & 0xFFFFFF00u) | (cur.x & 0x000000FFu);
                if (X + 8 == w)
                    d1 = (d1 & 0x00FFFFFFu) | (cur.y & 0xFF000000u);
            }
            const uint32_t n0 = noise_sub4(cur.x, d0), n1 = noise_sub4(cur.y, d1);
            if (all_rows || !(r & 1)) { /* wave-uniform */
                sum_d = __builtin_amdgcn_sad_u8(d0, 0u, sum_d), sum_d = __builtin_amdgcn_sad_u8(d1, 0u, sum_d);
                sum_n = __builtin_amdgcn_sad_u8(n0, 0u, sum_n), sum_n = __builtin_amdgcn_sad_u8(n1, 0u, sum_n);
                sq_d = __builtin_amdgcn_udot4(d0, d0, sq_d, false), sq_d = __builtin_amdgcn_udot4(d1, d1, sq_d, false);
                sq_n = __builtin_amdgcn_udot4(n0, n0, sq_n, false), sq_n = __builtin_amdgcn_udot4(n1, n1, sq_n, false);
            }
            prev = cur, cur = next;
        }
        /* ComputeMean / ComputeMeanOfSquaredValues of an 8x8 (C_DEFAULT/EbComputeMean_C.c:15, :45): (sum << 8) / 64 and (sum of squares << 16) / 64.
         * ComputeVariance64x64 takes its 8x8 values from rows 0, 2, 4, 6 on every path (ComputeSubMean8x8_SSE2_INTRIN, ComputeSubdMeanOfSquaredValues8x8_SSE2_INTRIN,
         * ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c:53, :10; ComputeIntermVarFour8x8_AVX2_INTRIN): sum << 3 and sum of squares << 11 */
        const int sm = all_rows ? 2 : 3, sq = all_rows ? 10 : 11;
        unsigned long long m_d = (unsigned long long)sum_d << sm, q_d = (unsigned long long)sq_d << sq;
        unsigned long long m_n = (unsigned long long)sum_n << sm, q_n = (unsigned long long)sq_n << sq;
#pragma unroll
        for (int l = 0; l < 3; l++)
            if (l < level) { /* wave-uniform: 16x16 (lanes ^1, ^8), 32x32 (^2, ^16), 64x64 (^4, ^32), each (a + b + c + d) >> 2 */
                m_d += __shfl_xor(m_d, 1 << l), q_d += __shfl_xor(q_d, 1 << l), m_n += __shfl_xor(m_n, 1 << l), q_n += __shfl_xor(q_n, 1 << l);
                m_d += __shfl_xor(m_d, 8 << l), q_d += __shfl_xor(q_d, 8 << l), m_n += __shfl_xor(m_n, 8 << l), q_n += __shfl_xor(q_n, 8 << l);
                m_d >>= 2, q_d >>= 2, m_n >>= 2, q_n >>= 2;
            }
        const unsigned long long var_d = q_d - m_d * m_d; /* unsigned, as written */
        /* the noise strip has no vertical term: the decimated methods read the block in rows 0 .. 15 (31) of the strip, i.e. the top rows of this 64x64 block */
        const unsigned long long var_n = __shfl(q_n - m_n * m_n, level == 3 ? lane : lane & 7);
        const int lead = level == 1 ? 9 : level == 2 ? 27 : 63; /* the lane at the origin of each block */
        if (!(lane & lead)) {
            const int per = 8 >> level; /* blocks = LCUs a side of this 64x64 block (lcuCodingOrder, :2978, :3122) */
            J.flat[(by64 * per + (by >> level)) * lcus_w + bx64 * per + (bx >> level)] = (var_d >> 16) < 50 && var_n > J.noise_th; /* FLAT_MAX_VAR(_DECIM) */
            term = var_n >> 16;
        }
        for (int o = 32; o > 0; o >>= 1)
            term += __shfl_xor(term, o);
    }
    if (lane == 0)
        s_term[wave] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = s_term[0] + s_term[1] + s_term[2] + s_term[3];
        if (t)
            atomicAdd(&J.red[blockIdx.x & (NOISE_PARTS - 1)], t);
    }
}

/* grid (pictures) */
__global__ __launch_bounds__(64) void k_noise_finish(const NoiseJobDev *__restrict__ jobs, int luma_height)
{
    const NoiseJobDev &J = jobs[blockIdx.x];
    if (threadIdx.x)
        return;
    unsigned long long sum = 0;
    for (int i = 0; i < NOISE_PARTS; i++)
        sum += J.red[i];
    /* totLcuCount: every 16x16 (32x32, 64x64) block inside the whole 64x64 blocks of the plane is complete and counted */
    const uint32_t count = (uint32_t)((J.w >> 6) * (J.h >> 6)) << (2 * (3 - J.level));
    const unsigned long long v = count ? sum / count : sum;
    uint32_t cls;
    if (J.method == SVT_AMD_NOISE_FULL) { /* :2635-2664: classes 4 .. 10 are folded back to 3_1 */
        const uint32_t th = luma_height <= 720 ? 25 : 0;
        cls = v >= 17 + th ? 4 : v >= 10 + th ? 3 : v >= 5 + th ? 2 : 1;
    } else if (J.method == SVT_AMD_NOISE_HALF) { /* :3171-3186 */
        const uint32_t th = luma_height <= 720 ? 25 : luma_height <= 1080 ? 10 : 0;
        cls = v >= 55 + th ? 4 : v >= 10 + th ? 3 : v >= 5 + th ? 2 : 1;
    } else { /* :3032-3042: noiseTh is 0, the top rung strict */
        cls = v > 60 ? 4 : v >= 10 ? 3 : v >= 5 ? 2 : 1;
    }
    SvtAmdNoisePic o;
    o.noise_variance_sum = sum, o.block_count = count, o.pic_noise_class = (uint8_t)cls;
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    *J.pic = o;
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

static size_t noise_flat_bytes(int w, int h) { return ((size_t)svt_amd_lcu_count(w, h) + 63) & ~(size_t)63; }

extern "C" size_t svt_amd_noise_detect_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    switch (which) {
    case SVT_AMD_NOISE_FLAT:
        return noise_flat_bytes(luma_width, luma_height);
    case SVT_AMD_NOISE_PICTURE:
        return sizeof(SvtAmdNoisePic);
    }
    return 0;
}

extern "C" int svt_amd_noise_detect_batch_launch(SvtAmdContext *ctx, const SvtAmdNoiseJob *jobs, int num_jobs, const SvtAmdNoiseArrays *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    if (!out->flat_noise || !out->picture)
        SVT_AMD_BAD("%s: job 0: there is no %s array", __func__, out->flat_noise ? "picture" : "flat_noise");
    int w = 0, h = 0;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdNoiseJob &j = jobs[i];
        SVT_AMD_TRY(svt_amd_batch_slot(__func__, ctx, i, j.cur_slot, &w, &h));
        if (j.method != SVT_AMD_NOISE_HALF && j.method != SVT_AMD_NOISE_QUARTER && j.method != SVT_AMD_NOISE_FULL)
            SVT_AMD_BAD("%s: job %d: noise detection method %d", __func__, i, j.method);
        if (j.noise_detection_th > 1)
            SVT_AMD_BAD("%s: job %d: noise detection threshold %d", __func__, i, j.noise_detection_th);
    }

    NoiseJobDev *d_tab;
    unsigned long long *d_red; /* the per-picture partial sums the block kernel accumulates into */
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_NOISE, sizeof(NoiseJobDev), NOISE_RED_BYTES, (void **)&d_tab, (void **)&d_red));
    const size_t b_flat = noise_flat_bytes(w, h);
    static thread_local NoiseJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    int max_blocks = 0;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdNoiseJob &j = jobs[i];
        const DevPicture *c = &ctx->slots[j.cur_slot];
        const DevPlane *pl = j.method == SVT_AMD_NOISE_FULL ? &c->full : j.method == SVT_AMD_NOISE_QUARTER ? &c->quarter : &c->sixteenth;
        NoiseJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        d.plane = pl->origin, d.pitch = pl->pitch, d.w = pl->width, d.h = pl->height;
        d.flat = out->flat_noise + (size_t)i * b_flat;
        d.pic = out->picture + i;
        d.red = d_red + (size_t)i * NOISE_PARTS;
        d.level = j.method == SVT_AMD_NOISE_FULL ? 3 : j.method == SVT_AMD_NOISE_QUARTER ? 2 : 1;
        d.noise_th = j.noise_detection_th == 1 ? 70000u : 120000u; /* the quarter method selects the same pair by the inverted test (:3002-3007) */
        d.method = j.method;
        const int blocks = (d.w >> 6) * (d.h >> 6);
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        SVT_AMD_TRY(svt_amd_batch_wait_slot(ctx, j.cur_slot));
    }
    /* the table goes up in stream order: a batch queued behind another one on this lane does not overwrite the table the first one still reads */
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(NoiseJobDev) * (size_t)num_jobs));
    /* the stages are ordered on the lane: a batch queued behind this one zeroes the partial sums only after this one's finish kernel has read them */
    HIP_TRY(hipMemsetAsync(d_red, 0, (size_t)num_jobs * NOISE_PARTS * 8, st));
    HIP_TRY(hipMemsetAsync(out->flat_noise, 0, (size_t)num_jobs * b_flat, st));
    if (max_blocks) /* a decimated picture below 64 samples a side: the reference's loops run zero blocks */
        hipLaunchKernelGGL(k_noise_blocks, dim3((unsigned)((max_blocks + 3) / 4), (unsigned)num_jobs), dim3(256), 0, st, (const NoiseJobDev *)d_tab, (w + 63) / 64);
    hipLaunchKernelGGL(k_noise_finish, dim3((unsigned)num_jobs), dim3(64), 0, st, (const NoiseJobDev *)d_tab, h);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
