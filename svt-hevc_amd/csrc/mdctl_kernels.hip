/*
 * mdctl_kernels.hip - the per-LCU controls of the mode decision (SvtAmdMdLcu, 191 bytes an LCU) assembled on the device from the records of the batches in front
 * of it, in the batched, stream-ordered shape of mdc_kernels.hip / irc_kernels.hip (include/svt_hevc_amd.h "Batched mode-decision LCU controls"):
 * what integration/svt_md_fill.h:svt_md_fill_lcu reads out of the reference's control sets on the host, with the reference functions it leans on restated -
 * DeriveContouringClass (Codec/EbModeDecisionConfiguration.c:395), ConfigureChroma (Codec/EbModeDecisionProcess.c:383), isEdgeLcu / isCompleteLcu
 * (Codec/EbSequenceControlSet.c:206-213), ConfigureLcuEdgeInfo (Codec/EbPictureControlSet.c:36).  Integer logic on records; no plane is read.  Restated as
 * tests/mdctl_numpy.py spells it out.
 *   k_mdctl_lcu     grid (LCUs / 4, pictures), a wave per LCU.  The record is built in 192 bytes of LDS per wave: the 171-byte head arrives as 43 words of the
 *                   SvtAmdMdcLcu record (a lane a word) - or, without one, the fixed leaf list is compacted into it as k_mdc_leaves does (mdc_units.h) - and
 *                   lane t < 20 computes byte 171 + t of the tail.  The records lie at byte alignment (191 is odd), so the wave stores the words of the ALIGNED
 *                   window around the record: lane b the word at (record & ~3) + 4 b, put together from four LDS bytes - 47 or 48 full words a record, the one or
 *                   two words the record shares with its neighbours as byte stores of its own bytes only.  Nothing outside the record is written; no atomics,
 *                   nothing to zero.
 *   k_mdctl_check   grid (1), a workgroup of 1024 threads: what svt_amd_md_encode_picture* has to know about a bound array before it launches
 *                   (SvtAmdMdCtlCheck) - the refusals of its host loop as counts and a first offender, the tile count.  A thread an LCU; a counter is a ballot
 *                   and a population count kept by one lane of each wave, the waves merged in LDS.
 * Bound: latency - 191 bytes written and about 400 read per LCU.
 */
#include "pa_batch.h"
#include "mdc_units.h"
#include "mdlaunch.h"
#include <string.h>
#define MD_FN __host__ __device__ __forceinline__
#include "md_logic.h"

struct MdCtlJobDev {
    const SvtAmdMdcLcu *mdc;       /* null: the fixed list of depth_mode 1 / 2 */
    const SvtAmdPaLcuStats *stats;
    const SvtAmdPaLcuDetect *detect;
    const SvtAmdSboLcu *sbo_lcu;
    const SvtAmdSboPic *sbo_pic;
    const SvtAmdIrcLcu *irc;       /* null (with energy): contouring class 0 */
    const uint64_t *energy;
    const uint8_t *stationary;     /* or null */
    const uint8_t *sticky;         /* or null */
    uint8_t *out;                  /* the picture's SvtAmdMdLcu[lcus] */
    uint16_t tile_cols, tile_rows;
    uint8_t depth_mode, chroma_level, cls, pan, tilt, c422, pad[6];
};
static_assert(sizeof(MdCtlJobDev) == 96, "MdCtlJobDev layout");
static_assert(sizeof(SvtAmdMdCtlJob) == 88 && sizeof(SvtAmdMdLcu) == 191 && sizeof(SvtAmdMdCtlCheck) == 88, "mode-decision control records");
static_assert(offsetof(SvtAmdMdLcu, tile_left) == 171 && offsetof(SvtAmdMdLcu, contouring_class) == 176 && offsetof(SvtAmdMdLcu, no_stop_split) == 187, "SvtAmdMdLcu layout");
static_assert(offsetof(SvtAmdMdcLcu, leaf_split) == offsetof(SvtAmdMdLcu, leaf_split) && offsetof(SvtAmdMdcLcu, lcu_md_mode) == 171 && offsetof(SvtAmdMdcLcu, aura_status) == 172,
              "the first 171 bytes of SvtAmdMdcLcu are the head of SvtAmdMdLcu");
#define MDCTL_HEAD 171
#define MDCTL_TAIL 20 /* bytes 171..190 */
#define MDCTL_CHECK_THREADS 1024
#define MDCTL_CHECK_WAVES (MDCTL_CHECK_THREADS / 64)
#define MDCTL_SLOTS 20 /* the counters of SvtAmdMdCtlCheck: md_mode[16], bad_leaf_count, bad_leaf_list, bad_chroma, tiles */

/* a tile starts at LCU column (row) x of n, x <= n: tileColStartLcu[c] = c * n / tiles == x for a c in 0..tiles (Codec/EbPictureControlSet.c:743).  tiles <= n, so
 * at most one c qualifies, and it is x * tiles / n or the next */
__device__ __forceinline__ bool mdctl_tile_start(int x, int n, int tiles)
{
    const int c = x * tiles / n;
    return c * n / tiles == x || (c + 1) * n / tiles == x;
}

/* grid (LCUs / 4, pictures): one wave per LCU */
__global__ __launch_bounds__(256) void k_mdctl_lcu(const MdCtlJobDev *__restrict__ jobs, int width, int height, int lcus_w, int lcus_h)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_rec[4][192];
    const MdCtlJobDev &J = jobs[blockIdx.y];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), b = threadIdx.x & 63;
    const int lcus = lcus_w * lcus_h, lcu = (int)blockIdx.x * 4 + wave;
    const bool active = lcu < lcus;
    const int n = active ? lcu : lcus - 1; /* a wave past the last LCU computes the last one again and stores nothing */
    const int col = n % lcus_w, row = n / lcus_w, ox = col * 64, oy = row * 64;
    uint8_t *rec = s_rec[wave];
    uint32_t *rec32 = (uint32_t *)rec;
    const bool listed = J.mdc != nullptr; /* workgroup-uniform */

    /* the head: bytes 0..171 of the configuration's record as 43 words (byte 171 is overwritten below), or zeroes under the fixed list */
    if (b < 48)
        rec32[b] = listed && b < 43 ? ((const uint32_t *)&J.mdc[n])[b] : 0u;
    int aura = 128, md_mode = 0; /* INVALID_AURA_STATUS: no aura detection ran */
    if (listed)
        aura = J.mdc[n].aura_status, md_mode = J.depth_mode == 0 ? J.mdc[n].lcu_md_mode : 0;
    __syncthreads();
    if (!listed) { /* Forward85 / 84CuToModeDecisionLCU as k_mdc_leaves has them: lane b speaks for units b and 64 + b; a valid unit from the first depth on */
        const int first = J.depth_mode == 1 ? 0 : 1;
        const int cu0 = b, cu1 = b < 21 ? 64 + b : 84;
        const MdcUnit u0 = mdc_unit(cu0), u1 = mdc_unit(cu1);
        const bool e0 = u0.depth >= first && ox + u0.x + (64 >> u0.depth) <= width && oy + u0.y + (64 >> u0.depth) <= height;
        const bool e1 = b < 21 && u1.depth >= first && ox + u1.x + (64 >> u1.depth) <= width && oy + u1.y + (64 >> u1.depth) <= height;
        const MdcSet emitted = mdc_set(e0, e1);
        const int count_lo = __popcll(emitted.lo);
        if (e0) {
            const int at = __popcll(emitted.lo & ((1ull << b) - 1ull));
            rec[1 + at] = (uint8_t)cu0, rec[86 + at] = u0.depth < 3;
        }
        if (e1) {
            const int at = count_lo + __popcll(emitted.hi & ((1ull << b) - 1ull));
            rec[1 + at] = (uint8_t)cu1, rec[86 + at] = u1.depth < 3;
        }
        if (b == 0)
            rec[0] = (uint8_t)(count_lo + __popcll(emitted.hi));
    }

    /* the tail: lane t computes byte 171 + t.  Everything but the four energies is wave-uniform */
    const SvtAmdPaLcuStats &S = J.stats[n];
    const SvtAmdPaLcuDetect &D = J.detect[n];
    const SvtAmdSboLcu &B = J.sbo_lcu[n];
    const int stationary = J.stationary ? J.stationary[n] : 0, sticky = J.sticky ? J.sticky[n] : 0;
    const bool complete = ox + 64 <= width && oy + 64 <= height;
    const bool edge = ox < 64 || oy < 64 || ox > width - 64 || oy > height - 64; /* isEdgeLcu: signed, as the promoted operands of the reference */
    /* ConfigureChroma */
    const bool high_luma = (sticky & 1) != 0 || B.high_luma != 0, high_chroma = (sticky & 2) != 0 || B.high_chroma != 0;
    const bool c0 = stationary != 0, c1 = D.homogeneous != 0 && high_chroma, c2 = !high_luma, c3 = J.sbo_pic->grass_percentage > 60 || aura == 1 || J.pan != 0;
    const int level = J.chroma_level;
    const bool full = level == 0 ? true : level == 1 ? false : level == 2 ? (c0 || c1 || c2) : level == 3 ? (c0 || c1) : level == 4 ? (c2 || c3) : c0;
    const int chroma = full && !J.c422 ? 1 : 2;
    /* DeriveContouringClass of leaf 1 + 21 q in lane 5 + q */
    const int t = b, q = (t - 5) & 3;
    int contour = 0;
    if (J.irc && t >= 5 && t < 9 && J.irc[n].homogeneous_over_time) {
        const unsigned long long e = J.energy[(size_t)n * 5 + 1 + q];
        contour = edge ? (e < 1024ull ? 2 : e < 3072ull ? 3 : 0) : (e < 256ull ? 1 : e < 1024ull ? 2 : e < 2048ull ? 3 : 0);
    }
    int v = 0;
    switch (t) {
    case 0: v = mdctl_tile_start(col, lcus_w, J.tile_cols); break;
    case 1: v = mdctl_tile_start(row, lcus_h, J.tile_rows); break;
    case 2: v = mdctl_tile_start(col + 1, lcus_w, J.tile_cols); break;
    case 3: v = complete; break;
    case 4: v = B.complex_lcu == 2; break;
    case 5: case 6: case 7: case 8: v = contour; break;
    case 9: v = chroma; break;
    case 10: v = (J.pan || J.tilt) && B.non_moving_index < 2 && S.y_mean[0] < 50; break;
    case 11: v = md_mode; break;
    case 12: v = aura == 0 && stationary == 0; break;
    case 13: v = B.cmplx_status == 4; break;
    case 14: v = S.variance[0] < 200; break;
    case 15: v = D.edge_block_num != 0; break;
    case 16: v = B.isolated_non_homogeneous != 0 || (J.cls < 3 && aura == 1); break;
    default: break; /* the pads */
    }
    if (t < MDCTL_TAIL + 1) /* ... and byte 191 of the wave's LDS, which is never stored */
        rec[MDCTL_HEAD + t] = (uint8_t)v;
    __syncthreads();

    /* the record leaves as the words of the aligned window around it */
    uint8_t *dst = J.out + (size_t)n * sizeof(SvtAmdMdLcu);
    const int o = 4 * b - (int)((uintptr_t)dst & 3u); /* the record offset of this lane's word: -3 .. 4 * 48 */
    if (active && o < (int)sizeof(SvtAmdMdLcu)) {
        if (o >= 0 && o + 4 <= (int)sizeof(SvtAmdMdLcu))
            *(uint32_t *)(dst + o) = (uint32_t)rec[o] | (uint32_t)rec[o + 1] << 8 | (uint32_t)rec[o + 2] << 16 | (uint32_t)rec[o + 3] << 24;
        else
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (o + k >= 0 && o + k < (int)sizeof(SvtAmdMdLcu))
                    dst[o + k] = rec[o + k];
    }
}

__device__ __forceinline__ uint32_t mdctl_wave_min(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

/* grid (1), a workgroup of 1024 threads: the summary of n records.  depth_mode: SvtAmdMdPicture.depth_mode; inter: the call applies md_lcu_supported */
__global__ __launch_bounds__(MDCTL_CHECK_THREADS) void k_mdctl_check(const SvtAmdMdLcu *__restrict__ lcus, int n, int depth_mode, int inter, SvtAmdMdCtlCheck *__restrict__ out)
{
    __shared__ uint32_t s_count[MDCTL_CHECK_WAVES][MDCTL_SLOTS], s_first[MDCTL_CHECK_WAVES];
    const int t = threadIdx.x, wave = t >> 6, b = t & 63;
    SvtAmdMdPicture P; /* md_lcu_supported reads the depth mode only */
    P.depth_mode = (uint8_t)depth_mode;
    uint32_t acc = 0, first = 0xFFFFFFFFu; /* lane s < MDCTL_SLOTS of a wave keeps the wave's counter s */
    for (int base = 0; base < n; base += MDCTL_CHECK_THREADS) { /* workgroup-uniform trip count: the ballots below see whole waves */
        const int i = base + t;
        const bool there = i < n;
        const SvtAmdMdLcu &L = lcus[there ? i : n - 1];
        const int count = L.leaf_count;
        const bool bad_count = count < 1 || count > SVT_AMD_MD_LEAVES;
        bool bad_list = false;
        int prev = -1;
        for (int k = 0; k < (count < SVT_AMD_MD_LEAVES ? count : SVT_AMD_MD_LEAVES); k++) {
            const int u = L.leaf_index[k];
            bad_list = bad_list || u >= SVT_AMD_MD_LEAVES || u <= prev;
            prev = u;
        }
        const int mode = L.lcu_md_mode < 15 ? L.lcu_md_mode : 15;
        const bool bad_chroma = L.chroma_encode_mode != 1 && L.chroma_encode_mode != 2;
        const bool tile = L.tile_left && L.tile_top;
        const bool unsupported = inter && !md_lcu_supported(&P, &L);
#pragma unroll
        for (int s = 0; s < MDCTL_SLOTS; s++) {
            const bool hit = s < 16 ? mode == s : s == 16 ? bad_count : s == 17 ? bad_list : s == 18 ? bad_chroma : tile;
            const uint32_t c = (uint32_t)__popcll(__ballot(there && hit));
            acc += b == s ? c : 0u;
        }
        if (there && first == 0xFFFFFFFFu && (bad_count || bad_list || unsupported)) /* the host loop's order within an LCU */
            first = (uint32_t)i << 2 | (bad_count ? 0u : bad_list ? 1u : 2u);
    }
    first = mdctl_wave_min(first);
    if (b < MDCTL_SLOTS)
        s_count[wave][b] = acc;
    if (b == 0)
        s_first[wave] = first;
    __syncthreads();
    if (t < MDCTL_SLOTS) {
        uint32_t sum = 0;
        for (int w = 0; w < MDCTL_CHECK_WAVES; w++)
            sum += s_count[w][t];
        uint32_t *slot = t < 16 ? &out->md_mode[t] : t == 16 ? &out->bad_leaf_count : t == 17 ? &out->bad_leaf_list : t == 18 ? &out->bad_chroma : &out->tiles;
        *slot = sum;
    }
    if (t == 32) {
        uint32_t f = 0xFFFFFFFFu;
        for (int w = 0; w < MDCTL_CHECK_WAVES; w++)
            f = min(f, s_first[w]);
        out->first_bad = f == 0xFFFFFFFFu ? f : f >> 2, out->first_kind = f == 0xFFFFFFFFu ? 0u : f & 3u;
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

extern "C" size_t svt_amd_md_controls_bytes(uint16_t luma_width, uint16_t luma_height, int which)
{
    return which == SVT_AMD_MDCTL_LCU ? (size_t)svt_amd_lcu_count(luma_width, luma_height) * sizeof(SvtAmdMdLcu) : 0;
}

/* the context's allocation: the descriptor table, then the check record of a bound array */
static int mdctl_begin(SvtAmdContext *ctx, MdCtlJobDev **d_tab, SvtAmdMdCtlCheck **d_check)
{
    void *tab, *scratch;
    SVT_AMD_TRY(svt_amd_batch_begin(ctx, BATCH_MDCTL, sizeof(MdCtlJobDev), sizeof(SvtAmdMdCtlCheck), &tab, &scratch));
    *d_tab = (MdCtlJobDev *)tab, *d_check = (SvtAmdMdCtlCheck *)scratch;
    return SVT_AMD_OK;
}

extern "C" int svt_amd_md_controls_batch_launch(SvtAmdContext *ctx, const SvtAmdMdCtlJob *jobs, int num_jobs, uint16_t luma_width, uint16_t luma_height, SvtAmdMdLcu *out)
{
    SVT_AMD_TRY(svt_amd_batch_header(__func__, ctx, jobs, out, num_jobs));
    /* ---- everything is checked before anything is queued ---- */
    SvtAmdBatchGeometry g;
    SVT_AMD_TRY(svt_amd_batch_geometry(__func__, ctx, luma_width, luma_height, SVT_AMD_MDCTL_MAX_LCUS, true, &g));
    const auto [w, h, wl, hl, lcus, groups, cap_lcus, cap_groups] = g;
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdMdCtlJob &j = jobs[i];
        if (!j.stats || !j.detect || !j.sbo_lcu || !j.sbo_pic)
            SVT_AMD_BAD("%s: job %d has no %s", __func__, i, !j.stats ? "block statistics" : !j.detect ? "detector records" : !j.sbo_lcu ? "source-ops LCU records" :
                        "source-ops picture record");
        if (j.slice_type > 2 || j.chroma_level > 5 || j.resolution_class > 3 || j.depth_mode > 5)
            SVT_AMD_BAD("%s: job %d: slice type %d, chroma level %d, resolution class %d, depth mode %d", __func__, i, j.slice_type, j.chroma_level, j.resolution_class,
                        j.depth_mode);
        if (!j.mdc_lcu && j.depth_mode != 1 && j.depth_mode != 2)
            SVT_AMD_BAD("%s: job %d has no mode-decision configuration records and depth mode %d (only 1 and 2 have a fixed leaf list)", __func__, i, j.depth_mode);
        if (!j.irc_lcu != !j.ac_energy)
            SVT_AMD_BAD("%s: job %d has %s but no %s", __func__, i, j.irc_lcu ? "initial rate control records" : "AC energies", j.irc_lcu ? "AC energies" :
                        "initial rate control records");
        if (j.tile_cols < 1 || j.tile_rows < 1 || j.tile_cols > wl || j.tile_rows > hl)
            SVT_AMD_BAD("%s: job %d: %d x %d tiles in a picture of %d x %d LCUs", __func__, i, j.tile_cols, j.tile_rows, wl, hl);
        if (j.pad0 || j.pad[0] || j.pad[1] || j.pad[2] || j.pad[3])
            SVT_AMD_BAD("%s: job %d: a pad byte is not 0", __func__, i);
    }

    MdCtlJobDev *d_tab;
    SvtAmdMdCtlCheck *d_check;
    SVT_AMD_TRY(mdctl_begin(ctx, &d_tab, &d_check));
    static thread_local MdCtlJobDev tab[SVT_AMD_MAX_BATCH];
    hipStream_t st = svt_amd_ctx_stream(ctx);
    for (int i = 0; i < num_jobs; i++) {
        const SvtAmdMdCtlJob &j = jobs[i];
        MdCtlJobDev &d = tab[i];
        memset(&d, 0, sizeof(d));
        d.mdc = j.mdc_lcu, d.stats = j.stats, d.detect = j.detect, d.sbo_lcu = j.sbo_lcu, d.sbo_pic = j.sbo_pic, d.irc = j.irc_lcu, d.energy = j.ac_energy;
        d.stationary = j.stationary_edge, d.sticky = j.sticky, d.out = (uint8_t *)(out + (size_t)i * lcus);
        d.tile_cols = j.tile_cols, d.tile_rows = j.tile_rows, d.depth_mode = j.depth_mode, d.chroma_level = j.chroma_level, d.cls = j.resolution_class;
        d.pan = j.is_pan != 0, d.tilt = j.is_tilt != 0, d.c422 = j.color_format_422_or_444 != 0;
    }
    SVT_AMD_TRY(svt_amd_upload_descriptors(ctx, d_tab, tab, sizeof(MdCtlJobDev) * (size_t)num_jobs));
    hipLaunchKernelGGL(k_mdctl_lcu, dim3((unsigned)groups, (unsigned)num_jobs), dim3(256), 0, st, (const MdCtlJobDev *)d_tab, w, h, wl, hl);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

/* svt_amd_internal.h */
int svt_amd_mdctl_check_async(SvtAmdContext *ctx, const SvtAmdMdLcu *d_lcus, int n, int depth_mode, int inter, SvtAmdMdCtlCheck *h_out)
{
    MdCtlJobDev *d_tab;
    SvtAmdMdCtlCheck *d_check;
    SVT_AMD_TRY(mdctl_begin(ctx, &d_tab, &d_check));
    hipStream_t st = svt_amd_ctx_stream(ctx);
    hipLaunchKernelGGL(k_mdctl_check, dim3(1), dim3(MDCTL_CHECK_THREADS), 0, st, d_lcus, n, depth_mode, inter, d_check);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_out, d_check, sizeof(*h_out), hipMemcpyDeviceToHost, st));
    return SVT_AMD_OK;
}

/* mdlaunch.h */
int svt_amd_mdctl_check_device(SvtAmdContext *ctx, const SvtAmdMdLcu *d_lcus, int n, int depth_mode, int inter, const SvtAmdMdCtlCheck **d_out)
{
    MdCtlJobDev *d_tab;
    SvtAmdMdCtlCheck *d_check;
    SVT_AMD_TRY(mdctl_begin(ctx, &d_tab, &d_check));
    hipLaunchKernelGGL(k_mdctl_check, dim3(1), dim3(MDCTL_CHECK_THREADS), 0, svt_amd_ctx_stream(ctx), d_lcus, n, depth_mode, inter, d_check);
    HIP_TRY(hipGetLastError());
    *d_out = d_check;
    return SVT_AMD_OK;
}

extern "C" int svt_amd_debug_md_controls_check(SvtAmdContext *ctx, const SvtAmdMdLcu *d_lcus, int n, int depth_mode, int inter, SvtAmdMdCtlCheck *out)
{
    if (!ctx || !d_lcus || !out || n < 1)
        SVT_AMD_BAD("%s: a context, a device array of at least one record and a place for the result", __func__);
    SVT_AMD_TRY(svt_amd_mdctl_check_async(ctx, d_lcus, n, depth_mode, inter != 0, out));
    HIP_TRY(hipStreamSynchronize(svt_amd_ctx_stream(ctx)));
    return SVT_AMD_OK;
}
