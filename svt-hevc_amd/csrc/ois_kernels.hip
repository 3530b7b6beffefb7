/*
 * Open-loop intra search on the device (SURVEY.md 8a front half, row "OpenLoopIntraSearchLcu").
 *
 * One workgroup (4 wavefronts) per LCU.  Replaces, per LCU, the reference's serial chain
 *   UpdateNeighborSamplesArrayOpenLoop -> IntraPredictionOpenLoop -> NxMSadKernel -> candidate injection
 * (EbMotionEstimation.c:5053-5320, EbIntraPrediction.c:5222-5421) by:
 *   1. the source window rows/cols -1..95 of the LCU in LDS (covers the 2N left / 2N top neighbours of every CU),
 *      and a transposed copy of the LCU's 64x64 samples,
 *   2. one wavefront per CU at a time (CU 1 + wave, 5 + wave, ...: every wave gets one 32x32 and four 16x16 CUs),
 *      an instance of the search per CU size: the CU's reference-sample array (out-of-picture samples = 128, no
 *      smoothing), its DC value and the main references of both angular classes, then a loop over the CU's modes
 *      (P/B: DC SAD -> GetOisPoint -> stage-1 modes, all inside the wave, no barrier); each mode is predicted four
 *      samples a lane: an angular mode is a row routine on packed bytes over the HEVC main reference (a negative
 *      angle adds its projected side samples), horizontal-class modes run the same routine against the transposed
 *      source; SAD by v_sad_u8 and wave reduction,
 *   3. per-CU decision threads reproducing the injection tables; the one serial dependency of the reference
 *      (bestMode / stage1SadArray surviving from CU to CU when no mode beats 32*32*255) is detected and, only
 *      then, replayed serially by one thread.
 * Results use the SvtAmdOisLcuResult convention (include/svt_hevc_amd.h): written bitfields flagged.
 */
#include "svt_amd_internal.h"

#define WIN_W 112 /* row pitch in bytes: columns -16 .. 95 of the LCU (seven 16-byte loads per row) */
#define WIN_X0 16 /* window column of LCU column 0 */
#define WIN_H 97
#define EXT_OFF 36 /* ext[EXT_OFF + k] = main[k], k = -N .. 2N+4 (the dword reads of a row reach 3 below the lowest index used) */
#define EXT_W 108

/* K = SAD columns per CU: 10 (intra: 7 modes; P/B: 9 stage-1 modes + DC in slot 9), 35 with ois_kernel_level */
template <int K> struct OisShared {
    union {
        struct {
            alignas(16) uint8_t win[WIN_H * WIN_W]; /* win[(y+1)*WIN_W + x + WIN_X0] = source sample (x,y) relative to the LCU */
            uint8_t wint[64 * 64];      /* wint[x*64 + y] = source sample (x,y), 0 <= x,y < 64 */
        } src;
        uint32_t out_cand[85][SVT_AMD_OIS_MAX_CAND]; /* decisions: written once the SADs are complete */
    } u;
    uint8_t refs[4][132];   /* per wave, its current CU: left[0..2N-1] top-to-bottom, top-left, top[0..2N-1] */
    uint8_t ext[4][2][EXT_W]; /* per wave, its current CU: the extended main reference of the vertical / horizontal class */
    uint32_t sad[85][K];
    uint8_t out_total[88];
    uint8_t nmodes[88];     /* stage-1 modes to test per CU (P path) */
    int stale;
};

__device__ __forceinline__ void cu_geom(int cu, int &x, int &y, int &N, int &lg)
{
    if (cu < 5)
        N = 32, lg = 5, x = ((cu - 1) & 1) * 32, y = ((cu - 1) >> 1) * 32;
    else if (cu < 21)
        N = 16, lg = 4, x = ((cu - 5) & 3) * 16, y = ((cu - 5) >> 2) * 16;
    else
        N = 8, lg = 3, x = ((cu - 21) & 7) * 8, y = ((cu - 21) >> 3) * 8;
}

__device__ __constant__ int8_t c_ang[9] = {0, 2, 5, 9, 13, 17, 21, 26, 32};
__device__ __constant__ int16_t c_inv[9] = {0, 4096, 1638, 910, 630, 482, 390, 315, 256};
__device__ __constant__ uint8_t c_islice[7] = {0, 1, 10, 26, 2, 18, 34};
__device__ __constant__ uint8_t c_stage1[9] = {10, 26, 2, 18, 34, 6, 14, 22, 30};
__device__ __constant__ uint8_t c_all35[35] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34};
__device__ __constant__ uint8_t c_inject[9][9] = {
    {10, 1, 0, 9, 11, 8, 12, 7, 13}, {26, 1, 0, 25, 27, 24, 28, 23, 29}, {2, 1, 0, 3, 4, 5, 7, 8, 9},
    {18, 1, 0, 17, 19, 16, 20, 15, 21}, {34, 1, 0, 33, 32, 29, 31, 27, 28}, {6, 1, 0, 7, 5, 4, 8, 3, 9},
    {14, 1, 0, 13, 15, 12, 16, 11, 17}, {22, 1, 0, 21, 23, 20, 24, 19, 25}, {30, 1, 0, 29, 31, 28, 32, 27, 33}};
__device__ __constant__ uint8_t c_isl_inject[5][3] = {{2, 4, 6}, {10, 6, 14}, {18, 14, 22}, {26, 22, 30}, {34, 32, 30}};
__device__ __constant__ int16_t c_ois_th[3][6][4] = {
    {{-20, 50, 150, 200}, {-20, 50, 150, 200}, {-20, 50, 100, 150}, {-20, 50, 200, 300}, {-20, 50, 200, 300}, {-20, 50, 200, 300}},
    {{-150, 0, 150, 200}, {-150, 0, 150, 200}, {-125, 0, 100, 150}, {-50, 50, 200, 300}, {-50, 50, 200, 300}, {-50, 50, 200, 300}},
    {{-400, -300, -200, 0}, {-400, -300, -200, 0}, {-400, -300, -200, 0}, {-400, -300, -200, 0}, {-400, -300, -200, 0}, {-400, -300, -200, 0}}};

/* planar / DC (with its N < 32 edge filter) of sample (x,y); r: left[0..2N-1], r[2N] = top-left, r[2N+1+j] = top[j] */
__device__ __forceinline__ int predict_planar_dc(int mode, int N, int lg, const uint8_t *r, int x, int y, int dc)
{
    const uint8_t *left = r, *top = r + 2 * N + 1;
    if (mode == 0)
        return ((N - 1 - x) * left[y] + (x + 1) * top[N] + (N - 1 - y) * top[x] + (y + 1) * left[N] + N) >> (lg + 1);
    if (N < 32) {
        if (x == 0 && y == 0)
            return (left[0] + top[0] + 2 * dc + 2) >> 2;
        if (y == 0)
            return (top[x] + 3 * dc + 2) >> 2;
        if (x == 0)
            return (left[y] + 3 * dc + 2) >> 2;
    }
    return dc;
}

/* wave sum on the DPP path (quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror: after the quad steps a mirror step completes the next power of two) and
 * v_readlane across the four rows: __shfl_xor compiles to ds_bpermute_b32, an LDS-crossbar round trip per step.  Wave-uniform result. */
#define OIS_DPP(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xF, 0xF, true))
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    v += OIS_DPP(v, 0xB1);
    v += OIS_DPP(v, 0x4E);
    v += OIS_DPP(v, 0x141);
    v += OIS_DPP(v, 0x140);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

/* LDS written by some lanes of a wave and read by others of the same wave */
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* one CU as seen by the wave that searches it */
template <int LG> struct CuView {
    int cx, cy;
    const uint8_t *r; /* reference samples (OisShared::refs[wave]) */
    uint8_t *ext;     /* OisShared::ext[wave]: the main reference of the vertical class, then of the horizontal class */
    int dc;
};

/* SAD of planar (mode 0) or DC (mode 1): four samples a lane, per-sample prediction only where it is not a constant */
template <int K, int LG>
__device__ __forceinline__ uint32_t sad_planar_dc(const OisShared<K> &S, const CuView<LG> &c, int mode, int lane)
{
    constexpr int N = 1 << LG, NQ = (N * N) >> 2, QS = LG - 2; /* dwords of the CU, log2 dwords per row */
    const uint32_t dc4 = (uint32_t)c.dc * 0x01010101u;
    uint32_t acc = 0;
#pragma unroll 1
    for (int q0 = 0; q0 < NQ; q0 += 64) {
        const int q = q0 + lane;
        if (NQ >= 64 || q < NQ) {
            const int y = q >> QS, x4 = (q & ((1 << QS) - 1)) << 2;
            const uint32_t sv = *(const uint32_t *)&S.u.src.win[(c.cy + y + 1) * WIN_W + c.cx + x4 + WIN_X0];
            uint32_t pv = dc4;
            if (mode == 0 || (N < 32 && (y == 0 || x4 == 0))) {
                pv = 0;
#pragma unroll
                for (int i = 0; i < 4; i++)
                    pv |= (uint32_t)predict_planar_dc(mode, N, LG, c.r, x4 + i, y, c.dc) << (8 * i);
            }
            acc = __builtin_amdgcn_sad_u8(sv, pv, acc);
        }
    }
    return wave_sum(acc);
}

/* SAD of an angular mode (2..34, 10 and 26 included), four samples a lane.
 * Vertical class (18..34): row y of the CU is, for every x, ((32-f)*main[x+i+1] + f*main[x+i+2] + 16) >> 5 with pos = (y+1)*angle, i = pos >> 5,
 * f = pos & 31 constant along the row; main[0] = top-left, main[k] = top[k-1], and for k < 0 the side (left) sample projected through the inverse
 * angle.  Horizontal class (2..17) is the same with left and top swapped and rows and columns swapped: it runs against the transposed source.
 * main[0 .. 2N] of both classes is built once per CU (search_cu); a negative angle adds its projected side samples below index 0.
 * The N < 32 edge filter of 10 / 26 touches column 0 of the (transposed) rows only and is patched in there. */
template <int K, int LG>
__device__ __forceinline__ uint32_t sad_angular(const OisShared<K> &S, const CuView<LG> &c, int mode, int lane)
{
    constexpr int N = 1 << LG, NQ = (N * N) >> 2, QS = LG - 2;
    const bool vert = mode >= 18;
    const int d = vert ? mode - 26 : 10 - mode; /* -8..8 */
    const int a = d < 0 ? -c_ang[-d] : c_ang[d];
    const uint8_t *left = c.r, *top = c.r + 2 * N + 1;
    const int tl = c.r[2 * N];
    const uint8_t *mainr = vert ? top : left, *side = vert ? left : top;
    uint8_t *ext = c.ext + (vert ? 0 : EXT_W);
    if (a < 0) { /* main[k] for kmin <= k < 0; kmin = ((N*a) >> 5) + 1 is the lowest index any sample reads */
        const int kmin = ((N * a) >> 5) + 1, k = -1 - lane;
        wave_lds_sync(); /* the previous mode's rows have read ext */
        if (k >= kmin)
            ext[EXT_OFF + k] = side[((-k * c_inv[-d] + 128) >> 8) - 1];
        wave_lds_sync();
    }

    const uint8_t *src = vert ? &S.u.src.win[(c.cy + 1) * WIN_W + c.cx + WIN_X0] : &S.u.src.wint[c.cx * 64 + c.cy];
    const int pitch = vert ? WIN_W : 64;
    const bool edge = N < 32 && d == 0;
    const uint32_t M = 0x00FF00FFu;
    uint32_t acc = 0;
#pragma unroll 1
    for (int q0 = 0; q0 < NQ; q0 += 64) {
        const int q = q0 + lane;
        if (NQ >= 64 || q < NQ) {
            const int v = q >> QS, u4 = (q & ((1 << QS) - 1)) << 2;
            const int pos = (v + 1) * a, i = pos >> 5, f = pos & 31;
            const int o = EXT_OFF + u4 + i + 1; /* main[u4 + i + 1] */
            const uint32_t *e32 = (const uint32_t *)&ext[o & ~3];
            const uint64_t w64 = (((uint64_t)e32[1] << 32) | e32[0]) >> ((o & 3) * 8); /* bytes B0..B4 = main[u4+i+1 .. u4+i+5] */
            const uint32_t w = (uint32_t)w64;
            const uint32_t p0 = w & M, p1 = (w >> 8) & M, p2 = (uint32_t)(w64 >> 16) & M; /* {B0,B2}, {B1,B3}, {B2,B4} */
            const uint32_t lo = ((p0 * (uint32_t)(32 - f) + p1 * (uint32_t)f + 0x00100010u) >> 5) & M;
            const uint32_t hi = ((p1 * (uint32_t)(32 - f) + p2 * (uint32_t)f + 0x00100010u) >> 5) & M;
            uint32_t pv = lo | (hi << 8);
            if (edge && u4 == 0)
                pv = (pv & ~0xFFu) | (uint32_t)min(255, max(0, mainr[0] + ((side[v] - tl) >> 1)));
            acc = __builtin_amdgcn_sad_u8(*(const uint32_t *)&src[v * pitch + u4], pv, acc);
        }
    }
    return wave_sum(acc);
}

template <int K, int LG>
__device__ __forceinline__ uint32_t mode_sad(const OisShared<K> &S, const CuView<LG> &c, int mode, int lane)
{
    return mode < 2 ? sad_planar_dc(S, c, mode, lane) : sad_angular(S, c, mode, lane);
}

/* the search of CU `cu` (N = 1 << LG) by one wave: references, DC, then the CU's modes (P/B: DC SAD -> GetOisPoint -> stage-1 modes) */
template <int K, int LG>
__device__ __forceinline__ void search_cu(OisShared<K> &S, const SvtAmdOisParams &P, const SvtAmdMeLcuResult *__restrict__ me, int lcu, int cu, int lx,
                                          int ly, bool wide, int wave, int lane)
{
    constexpr int N = 1 << LG;
    const int W = P.luma_width, H = P.luma_height;
    CuView<LG> c;
    int n_, lg_;
    cu_geom(cu, c.cx, c.cy, n_, lg_);
    const int ox = lx + c.cx, oy = ly + c.cy;
    if (ox + N > W || oy + N > H)
        return;
    uint8_t *R = S.refs[wave];
    wave_lds_sync(); /* the previous CU's modes have read R and ext */
    for (int e = lane; e < 4 * N + 1; e += 64) {
        int v = 128;
        if (e < 2 * N) {
            if (ox != 0 && oy + e < H)
                v = S.u.src.win[(c.cy + e + 1) * WIN_W + c.cx + WIN_X0 - 1];
        } else if (e == 2 * N) {
            if (ox != 0 && oy != 0)
                v = S.u.src.win[c.cy * WIN_W + c.cx + WIN_X0 - 1];
        } else {
            const int j = e - 2 * N - 1;
            if (oy != 0 && ox + j < W)
                v = S.u.src.win[c.cy * WIN_W + c.cx + j + WIN_X0];
        }
        R[e] = (uint8_t)v;
    }
    wave_lds_sync();
    /* main[0 .. 2N] of both classes (top-left, then top / left); main[2N+1 ..] is read with weight 0 only (angle 32) */
    uint8_t *ext = S.ext[wave][0];
    for (int e = lane; e < 2 * N + 5; e += 64) {
        ext[EXT_OFF + e] = e <= 2 * N ? R[2 * N + e] : 0;
        ext[EXT_W + EXT_OFF + e] = e == 0 ? R[2 * N] : e <= 2 * N ? R[e - 1] : 0;
    }
    wave_lds_sync();
    c.r = R;
    c.ext = ext;
    c.dc = (int)((wave_sum(lane < N ? (uint32_t)R[lane] + R[2 * N + 1 + lane] : 0u) + N) >> (LG + 1));

    const uint8_t *modes = c_islice; /* the modes to test, in SAD-slot order */
    int nk;
    if (P.slice_is_intra) {
        nk = N == 32 ? 1 : 7; /* 32x32: planar only */
    } else if (wide) {
        modes = c_all35, nk = 35;
    } else {
        const uint32_t dcSad = sad_planar_dc(S, c, 1, lane); /* DC -> slot 9 */
        if (lane == 0)
            S.sad[cu][9] = dcSad;
        if (P.limit_ois_to_dc_mode)
            return;
        /* GetInterIntraSadDistance / GetOisPoint (EbMotionEstimation.c:4782,4814) */
        const uint32_t meSad = me[lcu].pu[cu].distortion[0];
        const int32_t diff = (int32_t)((meSad - dcSad) * 100u);
        const int32_t dist = dcSad ? diff / (int32_t)dcSad : 0;
        int point = 4;
        const int16_t *th = c_ois_th[P.ois_th_set][P.temporal_layer_index];
        if (dcSad == 0 || meSad == 0 || dist <= th[0])
            point = 0;
        else if (dist <= th[1])
            point = 1;
        else if (dist <= th[2])
            point = 2;
        else if (dist <= th[3])
            point = 3;
        modes = c_stage1, nk = point == 0 ? 0 : 2 * point + 1;
        if (lane == 0)
            S.nmodes[cu] = (uint8_t)nk;
    }
    for (int k = 0; k < nk; k++) {
        const uint32_t s = mode_sad(S, c, modes[k], lane);
        if (lane == 0)
            S.sad[cu][k] = s;
    }
}

#define W_DIST (1u << 21)
#define W_VALID (1u << 22)
#define W_MODE (1u << 23)
__device__ __forceinline__ void set_dist(uint32_t &c, uint32_t d) { c = (c & ~0xFFFFFu) | (d & 0xFFFFFu) | W_DIST; }
__device__ __forceinline__ void set_valid(uint32_t &c, int v) { c = (c & ~(1u << 20)) | ((uint32_t)(v != 0) << 20) | W_VALID; }
__device__ __forceinline__ void set_mode(uint32_t &c, uint32_t m) { c = (c & 0x00FFFFFFu) | ((m & 0xFFu) << 24) | W_MODE; }

/* Decision step of one CU given its SADs (S.sad[cu][k], k = position in the tested mode list).
 * bestMode / stage1 carry the reference's function-scope state; returns false when the search of this CU did not
 * update bestMode (the caller must then replay serially). */
template <int K>
__device__ bool decide_cu(OisShared<K> &S, const SvtAmdOisParams &P, int cu, bool valid, uint32_t meSad, uint32_t &bestMode,
                          uint32_t *stage1)
{
    uint32_t *cand = S.u.out_cand[cu];
    for (int k = 0; k < SVT_AMD_OIS_MAX_CAND; k++)
        cand[k] = 0;
    S.out_total[cu] = 0xFF;
    int cx, cy, N, lg;
    cu_geom(cu, cx, cy, N, lg);
    bool updated = true;
    if (P.slice_is_intra) {
        for (int k = 0; k < 7; k++)
            set_valid(cand[k], 0);
        if (!valid)
            return true;
        if (N == 32) {
            set_dist(cand[0], S.sad[cu][0]);
            set_mode(cand[0], 0);
            set_valid(cand[0], 1);
            return true;
        }
        uint32_t best = 32 * 32 * 255;
        updated = false;
        for (int k = 0; k < 7; k++) {
            stage1[k] = S.sad[cu][k];
            if (stage1[k] < best)
                bestMode = c_islice[k], best = stage1[k], updated = true;
        }
        int count = 0;
        set_valid(cand[0], 1);
        set_dist(cand[0], stage1[0]);
        set_mode(cand[count++], 0);
        set_mode(cand[count++], 1);
        if (bestMode > 1) {
            const int g = bestMode == 2 ? 0 : bestMode == 10 ? 1 : bestMode == 18 ? 2 : bestMode == 26 ? 3 : 4;
            for (int k = 0; k < 3; k++)
                set_mode(cand[count++], c_isl_inject[g][k]);
        }
        S.out_total[cu] = (uint8_t)count;
        return updated;
    }
    if (!valid)
        return true;
    if (K >= 35 && P.ois_kernel_level) {
        for (int k = 0; k < 18; k++)
            set_valid(cand[k], 0);
        for (uint32_t m = 0; m < 35; m++) {
            const uint32_t sad = S.sad[cu][m];
            if (m < 18) {
                set_dist(cand[m], sad);
                set_mode(cand[m], m);
            } else {
                uint32_t worst = cand[0] & 0xFFFFFu, wi = 0;
                for (uint32_t k = 1; k < 18; k++)
                    if ((cand[k] & 0xFFFFFu) > worst)
                        worst = cand[k] & 0xFFFFFu, wi = k;
                if (sad < worst) {
                    set_dist(cand[wi], sad);
                    set_mode(cand[wi], m);
                }
            }
        }
        for (int i = 0; i < 18; i++)
            for (int j = i; j < 18; j++)
                if ((cand[i] & 0xFFFFFu) > (cand[j] & 0xFFFFFu)) {
                    const uint32_t mi = cand[i] >> 24, di = cand[i] & 0xFFFFFu;
                    set_mode(cand[i], cand[j] >> 24);
                    set_mode(cand[j], mi);
                    set_dist(cand[i], cand[j] & 0xFFFFFu);
                    set_dist(cand[j], di);
                }
        S.out_total[cu] = 18;
        return true;
    }
    for (int k = 0; k < 9; k++)
        set_valid(cand[k], 0);
    if (P.limit_ois_to_dc_mode) {
        set_dist(cand[0], S.sad[cu][9]);
        set_mode(cand[0], 1);
        set_valid(cand[0], 1);
        S.out_total[cu] = 1;
        return true;
    }
    stage1[0] = S.sad[cu][9]; /* DC SAD (slot 9) */
    const int n = S.nmodes[cu];
    if (n == 0) {
        set_mode(cand[0], 1);
        set_dist(cand[0], stage1[0]);
        S.out_total[cu] = 1;
        return true;
    }
    (void)meSad;
    uint32_t best = 32 * 32 * 255;
    updated = false;
    for (int k = 0; k < n; k++) {
        stage1[k] = S.sad[cu][k];
        if (stage1[k] < best)
            bestMode = c_stage1[k], best = stage1[k], updated = true;
    }
    int g = 8;
    for (int k = 0; k < 8; k++)
        if (bestMode == c_stage1[k])
            g = k;
    set_dist(cand[0], stage1[g]);
    set_valid(cand[0], P.set_best_ois_distortion_to_valid);
    for (int k = 0; k < 9; k++)
        set_mode(cand[k], c_inject[g][k]);
    S.out_total[cu] = (uint8_t)n;
    return updated;
}

/* K = 10: intra slices and the P/B stage-1 search (19.9 KB LDS, at most 64 VGPRs: 8 workgroups per CU); K = 35: a batch with a P/B picture under
 * ois_kernel_level (27.9 KB: 5 workgroups per CU) */
template <int K> __global__ __launch_bounds__(256, K >= 35 ? 5 : 8) void k_ois_picture(const OisJobDev *__restrict__ jobs)
{
    __shared__ OisShared<K> S;
    const OisJobDev &J = jobs[blockIdx.y];
    const int lcu = blockIdx.x;
    if (lcu >= J.nlcu)
        return;
    const SvtAmdOisParams P = J.P;
    const uint8_t *__restrict__ full = J.full;
    const int pitch = J.pitch, lcus_w = J.lcus_w;
    const SvtAmdMeLcuResult *__restrict__ me = J.me;
    SvtAmdOisLcuResult *__restrict__ out = J.out;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lx = (lcu % lcus_w) * 64, ly = (lcu / lcus_w) * 64;
    const int W = P.luma_width, H = P.luma_height;
    const bool wide = K >= 35 && !P.slice_is_intra && P.ois_kernel_level;
    const int last = P.slice_is_intra ? 84 : ((P.skip_ois_8x8 || P.cu8x8_mode == 1) ? 20 : 84);

    /* 1. window (the padded plane makes every address valid; out-of-picture samples are never USED): rows start at LCU column -16, a
     * 16-byte boundary of the plane, seven 16-byte loads per row */
    for (int i = t; i < WIN_H * 8; i += 256) {
        const int row = i >> 3, c16 = i & 7;
        if (c16 < 7)
            *(uint4 *)&S.u.src.win[row * WIN_W + c16 * 16] = *(const uint4 *)(full + (ptrdiff_t)(ly + row - 1) * pitch + lx - WIN_X0 + c16 * 16);
    }
    if (t == 0)
        S.stale = 0;
    __syncthreads();
    /* ... and its 64x64 samples transposed: a 4x4 block per thread */
    {
        const int x0 = (t & 15) << 2, y0 = (t >> 4) << 2;
        const uint8_t *w0 = &S.u.src.win[(y0 + 1) * WIN_W + x0 + WIN_X0];
        const uint32_t r0 = *(const uint32_t *)w0, r1 = *(const uint32_t *)(w0 + WIN_W), r2 = *(const uint32_t *)(w0 + 2 * WIN_W),
                       r3 = *(const uint32_t *)(w0 + 3 * WIN_W);
        const uint32_t a = __builtin_amdgcn_perm(r1, r0, 0x05010400u), b = __builtin_amdgcn_perm(r1, r0, 0x07030602u); /* {r0[0],r1[0],r0[1],r1[1]}, {..[2], ..[3]} */
        const uint32_t c = __builtin_amdgcn_perm(r3, r2, 0x05010400u), d = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
        uint8_t *o = &S.u.src.wint[x0 * 64 + y0];
        *(uint32_t *)o = __builtin_amdgcn_perm(c, a, 0x05040100u);
        *(uint32_t *)(o + 64) = __builtin_amdgcn_perm(c, a, 0x07060302u);
        *(uint32_t *)(o + 128) = __builtin_amdgcn_perm(d, b, 0x05040100u);
        *(uint32_t *)(o + 192) = __builtin_amdgcn_perm(d, b, 0x07060302u);
    }
    __syncthreads();

    /* 2. a wave per CU: CU 1 + wave, then 5 + wave, 9 + wave, ... */
    search_cu<K, 5>(S, P, me, lcu, 1 + wave, lx, ly, wide, wave, lane);
    for (int cu = 5 + wave; cu < 21; cu += 4)
        search_cu<K, 4>(S, P, me, lcu, cu, lx, ly, wide, wave, lane);
    if (last == 84)
        for (int cu = 21 + wave; cu < 85; cu += 4)
            search_cu<K, 3>(S, P, me, lcu, cu, lx, ly, wide, wave, lane);
    __syncthreads();

    /* 3. decisions: one thread per CU, then the serial replay if the carried state mattered (out_cand overlays the window) */
#define CU_VALID(cu_, v_)                                                          \
    do {                                                                           \
        int cx_, cy_, N_, lg_;                                                     \
        cu_geom(cu_, cx_, cy_, N_, lg_);                                           \
        v_ = !(lx + cx_ + N_ > W || ly + cy_ + N_ > H);                            \
    } while (0)
    if (t >= 1 && t <= 84) {
        if (t <= last) {
            bool valid;
            CU_VALID(t, valid);
            uint32_t bm = 0, st[11];
            for (int k = 0; k < 11; k++)
                st[k] = 0;
            if (!decide_cu(S, P, t, valid, 0, bm, st))
                S.stale = 1;
        } else {
            for (int k = 0; k < SVT_AMD_OIS_MAX_CAND; k++)
                S.u.out_cand[t][k] = 0;
            S.out_total[t] = 0xFF;
        }
    }
    if (t == 0) {
        for (int k = 0; k < SVT_AMD_OIS_MAX_CAND; k++)
            S.u.out_cand[0][k] = 0;
        S.out_total[0] = 0xFF;
    }
    __syncthreads();
    if (S.stale && t == 0) {
        uint32_t bm = 0, st[11];
        for (int k = 0; k < 11; k++)
            st[k] = 0;
        for (int cu = 1; cu <= last; cu++) {
            bool valid;
            CU_VALID(cu, valid);
            decide_cu(S, P, cu, valid, 0, bm, st);
        }
    }
    __syncthreads();

    /* 4. write the record */
    uint32_t *o = (uint32_t *)&out[lcu];
    const uint32_t *cs = &S.u.out_cand[0][0];
    for (int i = t; i < 85 * SVT_AMD_OIS_MAX_CAND; i += 256)
        o[i] = cs[i];
    uint8_t *ot = out[lcu].total_intra_luma_mode;
    if (t < 88)
        ot[t] = t < 85 ? S.out_total[t] : 0;
}

int svt_amd_launch_ois_batch(SvtAmdContext *ctx, const OisJobDev *host_jobs, int njobs, int max_lcus)
{
    {
        const int rcd = svt_amd_upload_descriptors(ctx, ctx->d_ois_jobs, host_jobs, sizeof(OisJobDev) * (size_t)njobs);
        if (rcd)
            return rcd;
    }
    bool wide = false; /* 35 SAD columns per CU only when some P/B picture of the batch ranks every mode */
    for (int i = 0; i < njobs; i++)
        wide |= !host_jobs[i].P.slice_is_intra && host_jobs[i].P.ois_kernel_level;
    if (wide)
        hipLaunchKernelGGL(k_ois_picture<35>, dim3(max_lcus, njobs), dim3(256), 0, svt_amd_ctx_stream(ctx), (const OisJobDev *)ctx->d_ois_jobs);
    else
        hipLaunchKernelGGL(k_ois_picture<10>, dim3(max_lcus, njobs), dim3(256), 0, svt_amd_ctx_stream(ctx), (const OisJobDev *)ctx->d_ois_jobs);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

/* ---------------------------------------------------------------------------------------------------
 * ComputeDecimatedZzSad (EbMotionEstimationProcess.c:176-300): one wavefront per LCU; the previous picture's
 * 1/16 plane IS the collocated LCU decimated by 4 (Decimation2D is a point sub-sampler), so both operands
 * come from the planes prep already built.  Lane = (row, 4-sample group): one v_sad_u8.
 * --------------------------------------------------------------------------------------------------- */
__global__ __launch_bounds__(256) void k_zz_sad(const uint8_t *__restrict__ cur16, const uint8_t *__restrict__ prev16,
                                                int pitch, int width, int height, int nlcu, int lcus_w,
                                                SvtAmdZzLcu *__restrict__ out)
{
    const int lcu = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (lcu >= nlcu)
        return;
    const int ox = (lcu % lcus_w) * 64, oy = (lcu / lcus_w) * 64;
    const int lw = min(64, width - ox), lh = min(64, height - oy);
    uint32_t sad = ~0u;
    uint8_t zz = 0xFF;
    if (lw == 64 && lh == 64) {
        const int r = lane >> 2, g = (lane & 3) << 2;
        const ptrdiff_t at = (ptrdiff_t)((oy >> 2) + r) * pitch + (ox >> 2) + g;
        const uint32_t s = __builtin_amdgcn_sad_u8(*(const uint32_t *)(cur16 + at), *(const uint32_t *)(prev16 + at), 0u);
        sad = wave_sum(s);
        zz = sad < 256 ? 0 : sad < 512 ? 3 : sad < 1024 ? 10 : sad < 2048 ? 20 : 30;
    }
    if (lane == 0) {
        const uint32_t area = (uint32_t)((lw >> 2) * (lh >> 2));
        SvtAmdZzLcu o;
        o.sad = sad, o.zz_cost = zz;
        o.non_moving_index = sad < area * 2 ? 0 : sad < area * 4 ? 10 : sad < area * 8 ? 20 : 30;
        o.pad[0] = o.pad[1] = 0;
        out[lcu] = o;
    }
}

int svt_amd_launch_zz_sad(SvtAmdContext *ctx, const DevPicture *cur, const DevPicture *prev, SvtAmdZzLcu *d_out)
{
    const int lw = (cur->width + 63) / 64, lh = (cur->height + 63) / 64;
    hipLaunchKernelGGL(k_zz_sad, dim3((lw * lh + 3) / 4), dim3(256), 0, svt_amd_ctx_stream(ctx), (const uint8_t *)cur->sixteenth.origin,
                       (const uint8_t *)prev->sixteenth.origin, (int)cur->sixteenth.pitch, (int)cur->width, (int)cur->height,
                       lw * lh, lw, d_out);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
