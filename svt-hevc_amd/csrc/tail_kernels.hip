/*
 * tail_kernels.hip - the picture tail on the device: deblocking, SAO and reference padding of an encoded picture from the contract records where they lie in HBM
 * (include/svt_hevc_amd.h "Picture tail on the device").  Two things live here.  The stream-ordered launch: nothing is uploaded, nothing is awaited, every
 * byte it works on is per picture object.  And the device chain itself (svt_amd_tail_queue_deblock / _sao / _reference, encdec_device.h), which the launch and the blocking
 * entries svt_amd_encdec_picture_deblock / _sao / _sao_decide / _reference (encdec_kernels.hip) both queue: those entries keep their checks, their host loops over the
 * records, their uploads and downloads and their waits, and nothing else.
 * What the reference does: the per-LCU deblocking drivers LCUInternalAreaDLFCore / LCUBoundaryDLFCore / LCUPictureEdgeDLFCore
 * (Codec/EbDeblockingFilter.c:2222, 2828, 3518, called from Codec/EbCodingLoop.c:4600-4631) on the boundary strengths of SetBSArrayBasedOnPUBoundary / TUBoundary
 * (:339, :472); SaoGenerationDecision[16bit] inside EncodePass (Codec/EbCodingLoop.c:4640-4750, Codec/EbSampleAdaptiveOffsetGenerationDecision.c:647-850, :936-1140) on
 * the picture as it stands when the LCU is done; ApplySaoOffsetsPicture (Codec/EbEncDecProcess.c:522-757); PadRefAndSetFlags (Codec/EbEncDecProcess.c:1805).
 *   k_tail_maps       grid (LCUs), 256 threads: the LCU's head and unit list staged in LDS (396 words), its tile of the three maps built in LDS by tail_logic.h
 *                     (gathered per cell, the later unit wins) and stored as whole rows; the flag bytes, the LCU's zeroed SvtAmdSaoLcuParams with its edge_flags and
 *                     its status byte; the LCU's source samples scattered into the three source planes, 16 bytes a lane where base and pitch allow.
 *   k_tail_check      grid (1): the status bytes reduced to one SvtAmdTailCheck.
 *   k_tail_composite  one launch for the three planes: the encoder-order view the SAO statistics are gathered on, 16 bytes a lane.
 *   k_tail_pad        one launch for the three planes: edge replication, the padded plane as one run of 16-byte stores.
 * No atomics, nothing zeroed beforehand.  Bound: HBM traffic - the source scatter reads and writes 1.5 samples a pixel, the composite reads 2 x and writes 1 x, the
 * padding reads and writes 1 x the padded picture.
 */
#include "encdec_device.h"
#include "pa_batch.h"
#define TAIL_FN __device__ static inline
#define TAIL_SYNC() __syncthreads()
#include "tail_logic.h"

static_assert(offsetof(SvtAmdLcuWork, lcu_x) == TAIL_W_LCU_X && offsetof(SvtAmdLcuWork, lcu_y) == TAIL_W_LCU_Y && offsetof(SvtAmdLcuWork, num_cus) == TAIL_W_NUM_CUS &&
              offsetof(SvtAmdLcuWork, tile_left) == TAIL_W_TILE_LEFT && offsetof(SvtAmdLcuWork, tile_top) == TAIL_W_TILE_TOP &&
              offsetof(SvtAmdLcuWork, tile_right) == TAIL_W_TILE_RIGHT && offsetof(SvtAmdLcuWork, cu) == TAIL_W_CU && offsetof(SvtAmdLcuWork, src_y) == TAIL_W_SRC &&
              offsetof(SvtAmdLcuWork16, cu) == TAIL_W_CU && offsetof(SvtAmdLcuWork16, src_y) == TAIL_W_SRC, "work record layout");
static_assert(sizeof(SvtAmdLcuCu) == TAIL_CU_BYTES && offsetof(SvtAmdLcuCu, size) == TAIL_CU_SIZE && offsetof(SvtAmdLcuCu, pred_mode) == TAIL_CU_MODE &&
              offsetof(SvtAmdLcuCu, qp) == TAIL_CU_QP && offsetof(SvtAmdLcuCu, inter_dir) == TAIL_CU_DIR && offsetof(SvtAmdLcuCu, mv) == TAIL_CU_MV, "unit layout");
static_assert(sizeof(SvtAmdLcuCuResult) == TAIL_R_CU_BYTES && offsetof(SvtAmdLcuCuResult, cbf) == 0 && offsetof(SvtAmdLcuResult, cu) == 0 &&
              offsetof(SvtAmdLcuResult16, cu) == 0 && SVT_AMD_LCU_MAX_CUS == TAIL_MAX_CUS, "result record layout");
static_assert(sizeof(SvtAmdCuMapEntry) == 12 && offsetof(SvtAmdCuMapEntry, dir) == 1 && offsetof(SvtAmdCuMapEntry, size_log2) == 2 && offsetof(SvtAmdCuMapEntry, mv) == 4,
              "map entry layout");
static_assert(sizeof(SvtAmdSaoLcuParams) == 72 && offsetof(SvtAmdSaoLcuParams, edge_flags) == 2, "SAO parameter layout");
static_assert(sizeof(SvtAmdTailCheck) == 16 && sizeof(TailCheckSums) == 16 && sizeof(SvtAmdTailJob) == 168, "tail records");
#define TAIL_PARAM_WORDS (sizeof(SvtAmdSaoLcuParams) / 4)

struct TailMapsArgs {
    const uint8_t *works, *results;
    size_t work_stride, result_stride;
    int width, height, lcu_cols, lcus;
    uint32_t *map;                 /* SvtAmdCuMapEntry[(height / 8) * (width / 8)] */
    uint8_t *cbf, *qp;             /* [(height / 4) * (width / 4)], [(height / 8) * (width / 8)] */
    uint8_t *edge, *sao_edge, *follow, *status; /* [lcus] each */
    uint32_t *lcu_params;          /* SvtAmdSaoLcuParams[lcus] */
    void *src[3];                  /* source planes, sample (0, 0) */
    int pitchY, pitchC;            /* samples */
    int vec;                       /* records and planes allow 16-byte accesses */
};

/* rows x cols samples of an LCU-local plane of pitch n (a power of two) into the picture plane */
template <typename T>
__device__ __forceinline__ void tail_scatter_plane(const T *__restrict__ src, int n, int rows, int cols, T *__restrict__ dst, int pitch, bool vec, int t)
{
    if (vec) {
        constexpr int N = 16 / (int)sizeof(T);
        const int cpr = n / N;
        for (int i = t; i < rows * cpr; i += 256) {
            const int y = i / cpr, x0 = (i - y * cpr) * N;
            if (x0 + N <= cols) {
                *reinterpret_cast<uint4 *>(dst + (size_t)y * pitch + x0) = *reinterpret_cast<const uint4 *>(src + y * n + x0);
            } else {
                for (int x = x0; x < cols; x++)
                    dst[(size_t)y * pitch + x] = src[y * n + x];
            }
        }
    } else {
        for (int i = t; i < rows * n; i += 256) {
            const int y = i / n, x = i - y * n;
            if (x < cols)
                dst[(size_t)y * pitch + x] = src[i];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_tail_maps(TailMapsArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_work[TAIL_W_SRC / 4];
    __shared__ TailTile s_tile;
    const int t = threadIdx.x, lcu = blockIdx.x;
    const uint8_t *work = A.works + (size_t)lcu * A.work_stride;
    for (int i = t; i < TAIL_W_SRC / 4; i += 256)
        s_work[i] = reinterpret_cast<const uint32_t *>(work)[i];
    const int below = lcu + A.lcu_cols < A.lcus ? A.works[(size_t)(lcu + A.lcu_cols) * A.work_stride + TAIL_W_TILE_TOP] : 0;
    __syncthreads();
    tail_lcu_build(reinterpret_cast<const uint8_t *>(s_work), A.results + (size_t)lcu * A.result_stride, below, lcu, A.lcu_cols, A.lcus, A.width, A.height, &s_tile, t, 256);

    /* the tile leaves as whole rows: the part of it inside the picture */
    const int lx8 = (lcu % A.lcu_cols) * 8, ly8 = (lcu / A.lcu_cols) * 8, w8 = A.width >> 3, h8 = A.height >> 3;
    const int cw = min(8, w8 - lx8), ch = min(8, h8 - ly8);
    if (t < 192) {
        const int r = t / 24, k = t - r * 24;
        if (r < ch && k < cw * 3)
            A.map[((size_t)(ly8 + r) * w8 + lx8) * 3 + k] = s_tile.map[r * 24 + k];
    }
    if (t < 64) {
        const int r = t >> 3, k = t & 7;
        if (r < ch && k < cw)
            A.qp[(size_t)(ly8 + r) * w8 + lx8 + k] = s_tile.qp[t];
    }
    {
        const int r = t >> 4, k = t & 15;
        if (r < 2 * ch && k < 2 * cw)
            A.cbf[(size_t)(2 * ly8 + r) * (2 * w8) + 2 * lx8 + k] = s_tile.cbf[t];
    }
    if (t == 0)
        A.edge[lcu] = s_tile.edge, A.sao_edge[lcu] = s_tile.sao_edge, A.follow[lcu] = s_tile.follow, A.status[lcu] = s_tile.status;
    if (t < (int)TAIL_PARAM_WORDS) /* the decision reads edge_flags and writes everything else */
        A.lcu_params[(size_t)lcu * TAIL_PARAM_WORDS + t] = t == 0 ? (uint32_t)s_tile.sao_edge << 16 : 0u;

    /* the LCU's source samples into the planes the SAO statistics read */
    if (s_tile.status & TAIL_LCU_BAD)
        return;
    const int ox = (lcu % A.lcu_cols) * 64, oy = (lcu / A.lcu_cols) * 64;
    const int lw = min(64, A.width - ox), lh = min(64, A.height - oy);
    const T *src = reinterpret_cast<const T *>(work + TAIL_W_SRC);
    const bool vec = A.vec != 0;
    tail_scatter_plane<T>(src, 64, lh, lw, (T *)A.src[0] + (size_t)oy * A.pitchY + ox, A.pitchY, vec, t);
    tail_scatter_plane<T>(src + 64 * 64, 32, lh >> 1, lw >> 1, (T *)A.src[1] + (size_t)(oy >> 1) * A.pitchC + (ox >> 1), A.pitchC, vec, t);
    tail_scatter_plane<T>(src + 64 * 64 + 32 * 32, 32, lh >> 1, lw >> 1, (T *)A.src[2] + (size_t)(oy >> 1) * A.pitchC + (ox >> 1), A.pitchC, vec, t);
}

/* grid (1): out_a (the picture object's copy) and out_b (the caller's, or null) */
__global__ __launch_bounds__(256) void k_tail_check(const uint8_t *__restrict__ status, int lcus, TailCheckSums *__restrict__ out_a, TailCheckSums *__restrict__ out_b)
{
    __shared__ TailCheckSums s_part[4];
    const int t = threadIdx.x;
    TailCheckSums a = tail_check_none();
    for (int i = t; i < lcus; i += 256)
        a = tail_check_add(a, (uint32_t)i, status[i]);
    for (int o = 32; o > 0; o >>= 1) {
        TailCheckSums b;
        b.bad_lcus = (uint32_t)__shfl_xor((int)a.bad_lcus, o), b.first_bad_lcu = (uint32_t)__shfl_xor((int)a.first_bad_lcu, o);
        b.bad_units = (uint32_t)__shfl_xor((int)a.bad_units, o), b.first_bad_unit_lcu = (uint32_t)__shfl_xor((int)a.first_bad_unit_lcu, o);
        a = tail_check_merge(a, b);
    }
    if ((t & 63) == 0)
        s_part[t >> 6] = a;
    __syncthreads();
    if (t == 0) {
        a = tail_check_merge(tail_check_merge(s_part[0], s_part[1]), tail_check_merge(s_part[2], s_part[3]));
        *out_a = a;
        if (out_b)
            *out_b = a;
    }
}

struct TailPlanes3 {
    const void *a[3], *b[3]; /* composite: deblocked, as encoded; padding: a = the stage */
    void *out[3];
    int pitchY, pitchC, width, height, lcu_cols;
    int ox, oy;              /* padding: luma */
    const uint8_t *follow;
};

/* The picture as the reference's SaoGenerationDecision sees each LCU (Codec/EbCodingLoop.c:4600-4750): the LCU's own deblocking drivers have run, those of the LCUs to its
 * right and below have not.  Those later drivers own the 8x8 filter blocks centred on the LCU boundary (LCUBoundaryDLFCore, Codec/EbDeblockingFilter.c:2828), i.e. every edge
 * segment inside the last 4 columns / rows of the LCU (in the plane's own samples) and nothing else inside it: the LCU is the deblocked picture with those strips still as
 * encoded, where a neighbour OF THE SAME TILE follows (at picture and tile edges the LCU's own LCUPictureEdgeDLFCore has finished them; follow: bit 0 right, bit 1 below).
 * (tests/test_oracle_encodepass_golden.py::test_encoder_order_sao_statistics_from_two_pictures proves it on the encoder's own records.)  grid (chunks of a luma row / 256, 2 * height): row y of the
 * grid is luma row y, then the Cb rows, then the Cr rows; a lane makes N samples (N a divisor of 32: a chunk lies in one LCU). */
template <typename T, int N>
__global__ __launch_bounds__(256) void k_tail_composite(TailPlanes3 P)
{
    const int gy = blockIdx.y, p = gy < P.height ? 0 : gy < P.height + (P.height >> 1) ? 1 : 2;
    const int y = p == 0 ? gy : p == 1 ? gy - P.height : gy - P.height - (P.height >> 1);
    const int pw = p ? P.width >> 1 : P.width, pitch = p ? P.pitchC : P.pitchY, lg = p ? 5 : 6, lcu = 1 << lg;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * N;
    if (x0 >= pw)
        return;
    const int f = P.follow[(y >> lg) * P.lcu_cols + (x0 >> lg)];
    const bool bottom = (y & (lcu - 1)) >= lcu - 4 && (f & 2), right = (f & 1) != 0;
    const size_t o = (size_t)y * pitch + x0;
    const T *dbk = (const T *)P.a[p] + o, *rec = (const T *)P.b[p] + o;
    T *out = (T *)P.out[p] + o;
    if (N > 1 && x0 + N <= pw) {
        typedef T Vec __attribute__((ext_vector_type(N)));
        const Vec d = *reinterpret_cast<const Vec *>(dbk), r = *reinterpret_cast<const Vec *>(rec);
        Vec v;
#pragma unroll
        for (int k = 0; k < N; k++)
            v[k] = (bottom || (right && ((x0 + k) & (lcu - 1)) >= lcu - 4)) ? r[k] : d[k];
        *reinterpret_cast<Vec *>(out) = v;
    } else {
        for (int k = 0; k < N && x0 + k < pw; k++)
            out[k] = (bottom || (right && ((x0 + k) & (lcu - 1)) >= lcu - 4)) ? rec[k] : dbk[k];
    }
}

/* PadRefAndSetFlags (Codec/EbEncDecProcess.c:1805; GeneratePadding / GeneratePadding16Bit): the finished picture inside a frame of replicated edge samples.  grid (chunks of the
 * padded luma plane / 256, 3): the padded plane is one run of samples, a lane makes N of them and stores them at once (the plane's start is 16-byte aligned). */
template <typename T, int N>
__global__ __launch_bounds__(256) void k_tail_pad(TailPlanes3 P)
{
    const int p = blockIdx.y, sh = p ? 1 : 0;
    const int pw = P.width >> sh, ph = P.height >> sh, ox = P.ox >> sh, oy = P.oy >> sh, stride = pw + 2 * ox, total = stride * (ph + 2 * oy);
    const int spitch = p ? P.pitchC : P.pitchY;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * N;
    if (i0 >= total)
        return;
    const T *src = (const T *)P.a[p];
    T *dst = (T *)P.out[p] + i0;
    int y = i0 / stride, x = i0 - y * stride;
    typedef T Vec __attribute__((ext_vector_type(N)));
    Vec v;
    if (x >= ox && x + N <= ox + pw) { /* the chunk lies inside the picture's columns of one row: one load (global memory takes the odd address) */
        __builtin_memcpy(&v, src + (size_t)min(max(y - oy, 0), ph - 1) * spitch + (x - ox), sizeof(v));
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) {
            v[k] = src[(size_t)min(max(y - oy, 0), ph - 1) * spitch + min(max(x - ox, 0), pw - 1)]; /* behind the plane's end: the last sample again, never stored */
            if (++x == stride)
                x = 0, y++;
        }
    }
    if (i0 + N <= total) {
        *reinterpret_cast<Vec *>(dst) = v;
    } else {
        for (int k = 0; k < N && i0 + k < total; k++)
            dst[k] = v[k];
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

/* the tail's working memory of one picture object: one allocation, carved up; freed with the object */
struct SvtAmdTailState {
    uint8_t *block;
    SvtAmdTailPointers p;          /* what the chain works on */
    uint8_t *sao_edge, *status;    /* [LCUs] each: k_tail_maps' other two bytes */
    TailCheckSums *check;
    bool maps_valid;               /* a tail has run on the object: svt_amd_debug_picture_tail_maps has something to fetch */
};

void svt_amd_tail_state_free(SvtAmdEncDecPicture *pic)
{
    SvtAmdTailState *s = pic->tail;
    if (!s)
        return;
    if (s->block)
        (void)hipFree(s->block);
    free(s);
    pic->tail = nullptr;
}

int svt_amd_tail_stage_planes(SvtAmdEncDecPicture *pic, bool dbk, bool fin, uint32_t origin_x, uint32_t origin_y)
{
    const uint32_t w = pic->d.width, h = pic->d.height, bps = pic->d.bps;
    for (int k = 0; k < 3; k++) {
        if (dbk && !pic->dbk[k] && hipMalloc((void **)&pic->dbk[k], pic->plane_bytes[k]) != hipSuccess) {
            svt_amd_set_error("hipMalloc (deblocked picture) failed");
            return SVT_AMD_ERR_RESOURCES;
        }
        if (fin && !pic->fin[k] && hipMalloc((void **)&pic->fin[k], pic->plane_bytes[k]) != hipSuccess) {
            svt_amd_set_error("hipMalloc (finished picture) failed");
            return SVT_AMD_ERR_RESOURCES;
        }
    }
    for (int k = 0; k < 3 && origin_x; k++) {
        const int sh = k ? 1 : 0;
        const size_t need = (size_t)((w >> sh) + 2 * (origin_x >> sh)) * ((h >> sh) + 2 * (origin_y >> sh)) * bps;
        if (pic->refp_bytes[k] < need) {
            if (pic->refp[k])
                HIP_TRY(hipFree(pic->refp[k]));
            pic->refp[k] = nullptr, pic->refp_bytes[k] = 0;
            if (hipMalloc((void **)&pic->refp[k], need) != hipSuccess) {
                svt_amd_set_error("hipMalloc (padded reference picture) failed");
                return SVT_AMD_ERR_RESOURCES;
            }
            pic->refp_bytes[k] = need;
        }
    }
    return SVT_AMD_OK;
}

static int tail_state(SvtAmdEncDecPicture *pic, bool with_fin, uint32_t origin_x, uint32_t origin_y)
{
    const uint32_t w = pic->d.width, h = pic->d.height;
    if (!pic->tail) {
        SvtAmdTailState *s = (SvtAmdTailState *)calloc(1, sizeof(*s));
        if (!s)
            return SVT_AMD_ERR_RESOURCES;
        auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
        const size_t n = (size_t)pic->nlcu, cells8 = (size_t)(w / 8) * (h / 8), cells4 = (size_t)(w / 4) * (h / 4);
        const size_t b_map = up(cells8 * sizeof(SvtAmdCuMapEntry)), b_cbf = up(cells4), b_qp = up(cells8), b_lcu = up(n), b_bs = n * 256, b_stats = up(sizeof(SvtAmdSaoStats) * n),
                     b_par = up(sizeof(SvtAmdSaoLcuParams) * n), b_cost = up(16 * n);
        size_t total = b_map + b_cbf + b_qp + 4 * b_lcu + 2 * b_bs + 3 * b_stats + b_par + b_cost + 256;
        for (int k = 0; k < 3; k++)
            total += 2 * up(pic->plane_bytes[k]);
        if (hipMalloc((void **)&s->block, total) != hipSuccess) {
            free(s);
            svt_amd_set_error("hipMalloc (picture tail state, %zu bytes) failed", total);
            return SVT_AMD_ERR_RESOURCES;
        }
        uint8_t *q = s->block;
        auto take = [&q](size_t bytes) { uint8_t *r = q; q += bytes; return r; };
        SvtAmdTailPointers &p = s->p;
        p.map = (uint32_t *)take(b_map), p.cbf = take(b_cbf), p.qp = take(b_qp);
        p.edge = take(b_lcu), s->sao_edge = take(b_lcu), p.follow = take(b_lcu), s->status = take(b_lcu);
        p.bsv = take(b_bs), p.bsh = take(b_bs);
        for (int k = 0; k < 3; k++)
            p.src[k] = take(up(pic->plane_bytes[k]));
        for (int k = 0; k < 3; k++)
            p.cmp[k] = take(up(pic->plane_bytes[k]));
        for (int k = 0; k < 3; k++)
            p.stats[k] = (SvtAmdSaoStats *)take(b_stats);
        p.stats_bytes = 3 * b_stats;
        p.par = (SvtAmdSaoLcuParams *)take(b_par), p.cost = (int64_t *)take(b_cost), s->check = (TailCheckSums *)take(256);
        pic->tail = s;
    }
    SVT_AMD_TRY(svt_amd_tail_stage_planes(pic, true, with_fin, origin_x, origin_y));
    if (!pic->ev_written && hipEventCreateWithFlags(&pic->ev_written, hipEventDisableTiming) != hipSuccess) {
        pic->ev_written = nullptr;
        return SVT_AMD_ERR_RESOURCES;
    }
    return SVT_AMD_OK;
}

extern "C" size_t svt_amd_picture_tail_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    if (luma_width < 1 || luma_height < 1)
        return 0;
    return which == SVT_AMD_TAIL_LCU_PARAMS ? (size_t)svt_amd_lcu_count(luma_width, luma_height) * sizeof(SvtAmdSaoLcuParams) : which == SVT_AMD_TAIL_CHECK ?
           sizeof(SvtAmdTailCheck) : 0;
}

extern "C" int svt_amd_encdec_picture_tail_warmup(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, uint32_t origin_x, uint32_t origin_y)
{
    if (!ctx || !pic)
        SVT_AMD_BAD("%s: a context and a picture object", __func__);
    if ((origin_x || origin_y) && !svt_amd_tail_origin_ok(origin_x, origin_y))
        SVT_AMD_BAD("%s: padding %u x %u (even, 8 to 256, or 0 x 0 for no reference planes)", __func__, origin_x, origin_y);
    HIP_TRY(hipSetDevice(ctx->device));
    return tail_state(pic, true, origin_x, origin_y);
}

extern "C" int svt_amd_encdec_picture_tail_launch(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdTailJob *job, SvtAmdSaoLcuParams *d_lcu_params,
                                                  SvtAmdTailCheck *d_check, SvtAmdRefPicture *ref)
{
    /* ---- everything is checked before anything is queued ---- */
    if (!ctx || !pic || !job)
        SVT_AMD_BAD("%s: a context, a picture object and a job", __func__);
    const uint32_t stages = job->stages;
    const bool deblock = stages & SVT_AMD_TAIL_DEBLOCK, decide = stages & SVT_AMD_TAIL_SAO_DECIDE, apply = stages & SVT_AMD_TAIL_SAO_APPLY, pad = stages & SVT_AMD_TAIL_REFERENCE;
    if (!stages || stages > 15u || job->pad)
        SVT_AMD_BAD("%s: stages 0x%x (SVT_AMD_TAIL_DEBLOCK 1, _SAO_DECIDE 2, _SAO_APPLY 4, _REFERENCE 8; pad %u is 0)", __func__, stages, job->pad);
    if (apply && !(decide && deblock))
        SVT_AMD_BAD("%s: SVT_AMD_TAIL_SAO_APPLY needs SVT_AMD_TAIL_SAO_DECIDE and SVT_AMD_TAIL_DEBLOCK in the same job (stages 0x%x)", __func__, stages);
    if (pad && (!ref || !svt_amd_tail_origin_ok(job->origin_x, job->origin_y)))
        SVT_AMD_BAD("%s: SVT_AMD_TAIL_REFERENCE needs `ref` and a padding of 8 to 256, even (%u x %u)", __func__, job->origin_x, job->origin_y);
    const bool maps = deblock || decide;
    const void *d_works = job->d_works, *d_results = job->d_results;
    size_t work_stride = job->work_stride, result_stride = job->result_stride;
    const uint32_t w = pic->d.width, h = pic->d.height, bps = pic->d.bps, wl = (w + 63) / 64, nlcu = (uint32_t)pic->nlcu;
    if (maps) {
        if (!d_works != !d_results)
            SVT_AMD_BAD("%s: work and result records come together (both device arrays, or both NULL for the records the object's last mode-decision call left)", __func__);
        if (!d_works) { /* the object form */
            if (pic->md_rect_n)
                SVT_AMD_BAD("%s: the picture object has a rank rectangle (svt_amd_encdec_picture_set_rect): the records of its other LCUs are zeroed", __func__);
            if (!pic->md_works_whole || !svt_amd_md_picture_records(pic, &d_works, &work_stride, &d_results, &result_stride))
                SVT_AMD_BAD("%s: no svt_amd_md_encode_picture* call that writes work records has completed on the picture object", __func__);
        }
        const size_t work_min = bps == 2 ? sizeof(SvtAmdLcuWork16) : sizeof(SvtAmdLcuWork), result_min = bps == 2 ? sizeof(SvtAmdLcuResult16) : sizeof(SvtAmdLcuResult);
        if (work_stride < work_min || work_stride % 4 || (uintptr_t)d_works % 4)
            SVT_AMD_BAD("%s: work records %zu bytes apart at %p (words; at least the %zu bytes of the object's sample width)", __func__, work_stride, d_works, work_min);
        if (result_stride < result_min || result_stride % 4 || (uintptr_t)d_results % 4)
            SVT_AMD_BAD("%s: result records %zu bytes apart at %p (words; at least the %zu bytes of the object's sample width)", __func__, result_stride, d_results, result_min);
    }
    if (!pic->written)
        SVT_AMD_BAD("%s: the picture object holds no encoded picture", __func__);
    if (pic->d.pitch[1] != pic->d.pitch[2])
        SVT_AMD_BAD("%s: the chroma planes differ in pitch", __func__);
    if (deblock && (job->deblock.slice_type > 3 || job->deblock.pad[0] || job->deblock.pad[1] || job->deblock.pad[2]))
        SVT_AMD_BAD("%s: deblocking parameters: slice type %d, pad bytes 0", __func__, job->deblock.slice_type);
    if ((uintptr_t)d_lcu_params % 4 || (uintptr_t)d_check % 4)
        SVT_AMD_BAD("%s: the parameters at %p or the check record at %p (4-byte aligned)", __func__, (void *)d_lcu_params, (void *)d_check);

    HIP_TRY(hipSetDevice(ctx->device));
    SVT_AMD_TRY(tail_state(pic, apply, pad ? job->origin_x : 0, pad ? job->origin_y : 0));
    SvtAmdTailState *s = pic->tail;
    hipStream_t st = svt_amd_ctx_stream(ctx);
    const int pY = (int)pic->d.pitch[0], pC = (int)pic->d.pitch[1];

    if (maps) {
        TailMapsArgs A;
        A.works = (const uint8_t *)d_works, A.results = (const uint8_t *)d_results, A.work_stride = work_stride, A.result_stride = result_stride;
        A.width = (int)w, A.height = (int)h, A.lcu_cols = (int)wl, A.lcus = (int)nlcu;
        A.map = s->p.map, A.cbf = s->p.cbf, A.qp = s->p.qp, A.edge = s->p.edge, A.sao_edge = s->sao_edge, A.follow = s->p.follow, A.status = s->status;
        A.lcu_params = (uint32_t *)s->p.par;
        for (int k = 0; k < 3; k++)
            A.src[k] = s->p.src[k];
        A.pitchY = pY, A.pitchC = pC;
        A.vec = !((uintptr_t)d_works % 16) && !(work_stride % 16) && !((size_t)pY * bps % 16) && !((size_t)pC * bps % 16);
        if (bps == 1)
            hipLaunchKernelGGL(k_tail_maps<uint8_t>, dim3(nlcu), dim3(256), 0, st, A);
        else
            hipLaunchKernelGGL(k_tail_maps<uint16_t>, dim3(nlcu), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_tail_check, dim3(1), dim3(256), 0, st, (const uint8_t *)s->status, (int)nlcu, s->check, (TailCheckSums *)d_check);
        HIP_TRY(hipGetLastError());
        s->maps_valid = true;
    }
    if (deblock)
        SVT_AMD_TRY(svt_amd_tail_queue_deblock(ctx, pic, s->p, &job->deblock));
    if (decide) { /* the composite is of this job's deblocking: without it the picture as encoded is looked at (allowEncDecMismatch) */
        SVT_AMD_TRY(svt_amd_tail_queue_sao(ctx, pic, s->p, &job->sao, job->d_sao_enable, deblock, apply));
        if (d_lcu_params)
            HIP_TRY(hipMemcpyAsync(d_lcu_params, s->p.par, sizeof(SvtAmdSaoLcuParams) * (size_t)nlcu, hipMemcpyDeviceToDevice, st));
    }
    if (pad)
        SVT_AMD_TRY(svt_amd_tail_queue_reference(ctx, pic, job->origin_x, job->origin_y, ref));
    return ep_picture_written(ctx, pic);
}

/* ---- the device chain: what the launch above and the blocking entries (encdec_kernels.hip) queue; everything they work on is in `p` and the object's stages.  (Below the
 * launch, so that the compiler meets the kernels in the order k_tail_maps, k_tail_check, k_tail_composite, k_tail_pad and the code object keeps its layout.) ---- */

int svt_amd_tail_queue_deblock(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdTailPointers &p, const SvtAmdDeblockParams *prm)
{
    const uint32_t w = pic->d.width, h = pic->d.height;
    SVT_AMD_TRY(svt_amd_bs_picture(ctx, (const SvtAmdCuMapEntry *)p.map, p.cbf, w, h, prm->slice_type, prm->ref_poc[0], prm->ref_poc[1], p.edge, p.bsv, p.bsh));
    /* the deblocked picture is a second set of planes: the picture as encoded stays (the neighbours of LCUs still to come, and the part of the SAO statistics that the
     * reference gathers before an LCU's right / bottom edges are filtered: k_tail_composite) */
    for (int k = 0; k < 3; k++)
        HIP_TRY(hipMemcpyAsync(pic->dbk[k], pic->d.rec[k], pic->plane_bytes[k], hipMemcpyDeviceToDevice, svt_amd_ctx_stream(ctx)));
    SVT_AMD_TRY(svt_amd_dlf_picture(ctx, (int)pic->d.bps, pic->dbk[0], pic->d.pitch[0], pic->dbk[1], pic->dbk[2], pic->d.pitch[1], w, h, p.bsv, p.bsh, p.qp, w / 8, prm->tc_offset,
                                    prm->beta_offset, prm->cb_qp_offset, prm->cr_qp_offset));
    pic->deblocked = true;
    return SVT_AMD_OK;
}

int svt_amd_tail_queue_sao(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdTailPointers &p, const SvtAmdSaoDecisionParams *prm, const uint8_t *d_enable, bool composite,
                           bool apply)
{
    const uint32_t w = pic->d.width, h = pic->d.height, bps = pic->d.bps, wl = (w + 63) / 64, hl = (h + 63) / 64;
    const int pY = (int)pic->d.pitch[0], pC = (int)pic->d.pitch[1];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    HIP_TRY(hipMemsetAsync(p.stats[0], 0, p.stats_bytes, st));
    if (composite) {
        TailPlanes3 P;
        memset(&P, 0, sizeof(P));
        for (int k = 0; k < 3; k++)
            P.a[k] = pic->dbk[k], P.b[k] = pic->d.rec[k], P.out[k] = p.cmp[k];
        P.pitchY = pY, P.pitchC = pC, P.width = (int)w, P.height = (int)h, P.lcu_cols = (int)wl, P.follow = p.follow;
        if (bps == 1)
            hipLaunchKernelGGL((k_tail_composite<uint8_t, 16>), dim3(((w + 15) / 16 + 255) / 256, 2 * h), dim3(256), 0, st, P);
        else
            hipLaunchKernelGGL((k_tail_composite<uint16_t, 8>), dim3(((w + 7) / 8 + 255) / 256, 2 * h), dim3(256), 0, st, P);
        HIP_TRY(hipGetLastError());
    }
    /* GatherSaoStatisticsLcu* of the components the mode looks at (EbSampleAdaptiveOffsetGenerationDecision.c:647-760); a picture without a composite (never deblocked:
     * allowEncDecMismatch, a decide-only call) is its own encoder-order view */
    const int ncomp = prm->mm_sao ? 3 : (prm->temporal_layer < 2 ? 1 : 0);
    for (int k = 0; k < ncomp; k++)
        SVT_AMD_TRY(svt_amd_sao_gather_picture(ctx, (int)bps, p.src[k], k ? pC : pY, composite ? (const void *)p.cmp[k] : (const void *)pic->d.rec[k], k ? pC : pY, k ? w / 2 : w,
                                               k ? h / 2 : h, k ? 32 : 64, prm->mm_sao ? 0 : 1, p.stats[k]));
    SVT_AMD_TRY(svt_amd_sao_decide_picture(ctx, prm, p.stats[0], p.stats[1], p.stats[2], wl, hl, d_enable, p.par, p.cost));
    if (apply) {
        const void *srcs[3] = {pic->dbk[0], pic->dbk[1], pic->dbk[2]};
        void *dsts[3] = {pic->fin[0], pic->fin[1], pic->fin[2]};
        SVT_AMD_TRY(svt_amd_sao_apply_picture(ctx, (int)bps, srcs, dsts, pic->d.pitch[0], pic->d.pitch[1], w, h, p.par, 1, 1));
        pic->sao_done = true;
    }
    return SVT_AMD_OK;
}

int svt_amd_tail_queue_reference(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, uint32_t origin_x, uint32_t origin_y, SvtAmdRefPicture *ref)
{
    const uint32_t w = pic->d.width, h = pic->d.height, bps = pic->d.bps;
    uint8_t *const *stage = pic->sao_done ? pic->fin : pic->deblocked ? pic->dbk : pic->d.rec;
    TailPlanes3 P;
    memset(&P, 0, sizeof(P));
    for (int k = 0; k < 3; k++)
        P.a[k] = stage[k], P.out[k] = pic->refp[k];
    P.pitchY = (int)pic->d.pitch[0], P.pitchC = (int)pic->d.pitch[1], P.width = (int)w, P.height = (int)h, P.ox = (int)origin_x, P.oy = (int)origin_y;
    const uint32_t total = (w + 2 * origin_x) * (h + 2 * origin_y), n = 16 / bps, chunks = (total + n - 1) / n;
    if (bps == 1)
        hipLaunchKernelGGL((k_tail_pad<uint8_t, 16>), dim3((chunks + 255) / 256, 3), dim3(256), 0, svt_amd_ctx_stream(ctx), P);
    else
        hipLaunchKernelGGL((k_tail_pad<uint16_t, 8>), dim3((chunks + 255) / 256, 3), dim3(256), 0, svt_amd_ctx_stream(ctx), P);
    HIP_TRY(hipGetLastError());
    ref->d_y = pic->refp[0], ref->d_cb = pic->refp[1], ref->d_cr = pic->refp[2];
    ref->strideY = w + 2 * origin_x, ref->strideC = (w >> 1) + 2 * (origin_x >> 1), ref->originX = origin_x, ref->originY = origin_y;
    ref->width = w, ref->height = h;
    return SVT_AMD_OK;
}

/* debug / test: what the object's last tail derived from the records; every pointer HOST and optional.  lcu_bytes: [4][LCUs] - the deblocking edge byte, the SAO edge
 * flags, the follow bits, the status byte; src_*: the source planes, tightly packed.  Blocking. */
extern "C" int svt_amd_debug_picture_tail_maps(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, SvtAmdCuMapEntry *map, uint8_t *cbf, uint8_t *qp, uint8_t *lcu_bytes,
                                               SvtAmdTailCheck *check, void *src_y, void *src_cb, void *src_cr)
{
    if (!ctx || !pic)
        SVT_AMD_BAD("%s: a context and a picture object", __func__);
    if (!pic->tail || !pic->tail->maps_valid)
        SVT_AMD_BAD("%s: no svt_amd_encdec_picture_tail_launch with a filter stage has run on the picture object", __func__);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    const SvtAmdTailState *s = pic->tail;
    const size_t w = pic->d.width, h = pic->d.height, n = (size_t)pic->nlcu, bps = pic->d.bps;
    if (map)
        HIP_TRY(hipMemcpy(map, s->p.map, (w / 8) * (h / 8) * sizeof(SvtAmdCuMapEntry), hipMemcpyDeviceToHost));
    if (cbf)
        HIP_TRY(hipMemcpy(cbf, s->p.cbf, (w / 4) * (h / 4), hipMemcpyDeviceToHost));
    if (qp)
        HIP_TRY(hipMemcpy(qp, s->p.qp, (w / 8) * (h / 8), hipMemcpyDeviceToHost));
    const uint8_t *bytes[4] = {s->p.edge, s->sao_edge, s->p.follow, s->status};
    for (int k = 0; k < 4 && lcu_bytes; k++)
        HIP_TRY(hipMemcpy(lcu_bytes + k * n, bytes[k], n, hipMemcpyDeviceToHost));
    if (check)
        HIP_TRY(hipMemcpy(check, s->check, sizeof(*check), hipMemcpyDeviceToHost));
    void *outs[3] = {src_y, src_cb, src_cr};
    for (int k = 0; k < 3; k++)
        if (outs[k]) {
            const size_t pw = k ? w / 2 : w, ph = k ? h / 2 : h;
            HIP_TRY(hipMemcpy2D(outs[k], pw * bps, s->p.src[k], (size_t)pic->d.pitch[k] * bps, pw * bps, ph, hipMemcpyDeviceToHost));
        }
    return SVT_AMD_OK;
}
