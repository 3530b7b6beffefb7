/* coeffscan_device.h - the per-LCU digest of the entropy hand-off pre-scan as device functions, for the kernels of handoff_kernels.hip (counted, then written in
 * place): the block table of an LCU's units, the workgroup scan, the 4x4 scans, the digest of a sub-block's 16 values in registers and the per-block lists (last
 * sub-block, groups, levels, the SvtAmdCoeffScanTu record).  What each step restates of EncodeQuantizedCoefficients (Codec/EbEntropyCoding.c:1172) is said where it
 * stands. */
#ifndef SVT_AMD_COEFFSCAN_DEVICE_H
#define SVT_AMD_COEFFSCAN_DEVICE_H
#include <stddef.h>
#include "rate_device.h"
#include "svt_amd_internal.h"

#define CS_MAX_TUS (3 * SVT_AMD_LCU_MAX_CUS)
#define CS_MAX_SUBS 384
#define CS_MAX_LEVELS 6144

struct CsTu {
    uint16_t coeff_off;   /* first coefficient in its plane (LCU-local) */
    uint8_t plane, lg, scan, valid;
    uint16_t nz;          /* the unit's recorded count (nzCoefCount) */
    uint16_t sub_base;    /* first sub-block in the LCU's sub-block index space */
    int16_t last;
    uint16_t first_group, level_base;
};

struct CsShared {
    CsTu tu[CS_MAX_TUS];
    uint16_t scan_in[256];                  /* scratch of the block-wide scans */
    uint16_t wave_tot[4];
    uint8_t owner[CS_MAX_SUBS];             /* block of a sub-block index */
    uint16_t sig[CS_MAX_SUBS];
    uint8_t cnt[CS_MAX_SUBS];
    uint16_t lvl_off[CS_MAX_SUBS];          /* first level of the sub-block in the LCU's list */
    int16_t grp[CS_MAX_SUBS];               /* its group in the LCU's list, -1 = beyond the last sub-block */
    uint32_t total_subs, total_groups, total_levels;
};

/* exclusive scan of one value per thread over the 256 threads; returns this thread's prefix, *total = sum */
__device__ __forceinline__ uint32_t cs_scan256(CsShared &S, uint32_t v, uint32_t *total)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d)
            x += y;
    }
    if (lane == 63)
        S.wave_tot[wave] = (uint16_t)x;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave)
            base += S.wave_tot[w];
        sum += S.wave_tot[w];
    }
    __syncthreads();
    *total = sum;
    return base + x - v;
}

/* the 16 values of a sub-block in forward scan order k = 0..15: which raster position (y * 4 + x) scan position k reads.  Diagonal: up-right
 * diagonals (H.265 6.5.3); horizontal: raster; vertical: column by column - the reference's scans4 tables with its x / y swap of SCAN_HOR2 folded
 * in (:1398-1410). */
__device__ __forceinline__ int cs_raster_of(int scan, int k)
{
    constexpr uint8_t diag[16] = {0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15};
    return scan == 0 ? diag[k] : scan == 1 ? k : ((k & 3) << 2) | (k >> 2);
}

struct CsSub {
    uint32_t sig, cnt, sign, gt1;
    uint16_t level[16]; /* coding order; [0, cnt) valid */
};

template <int SCAN>
__device__ __forceinline__ void cs_digest(const int16_t (&v)[16], CsSub &o)
{
    o.sig = 0, o.cnt = 0, o.sign = 0, o.gt1 = 0;
#pragma unroll
    for (int k = 0; k < 16; k++)
        o.sig |= (uint32_t)(v[cs_raster_of(SCAN, k)] != 0) << k;
    /* coded coefficients: the set positions from the top down */
#pragma unroll
    for (int i = 0; i < 16; i++)
        o.level[i] = 0;
#pragma unroll
    for (int k = 15; k >= 0; k--) {
        const int c = v[cs_raster_of(SCAN, k)];
        if (c != 0) {
            const uint32_t a = (uint32_t)(c < 0 ? -c : c);
            o.sign = o.sign * 2 + (c < 0);
            o.gt1 |= (uint32_t)(a > 1) << o.cnt;
            /* level[cnt] = a without a dynamically indexed register array: a select per slot */
#pragma unroll
            for (int i = 0; i < 16; i++)
                o.level[i] = (uint32_t)i == o.cnt ? (uint16_t)a : o.level[i];
            o.cnt++;
        }
    }
}
__device__ __forceinline__ void cs_digest_scan(int scan, const int16_t (&v)[16], CsSub &o)
{
    if (scan == 0)
        cs_digest<0>(v, o);
    else if (scan == 1)
        cs_digest<1>(v, o);
    else
        cs_digest<2>(v, o);
}
/* the significance map alone (forward scan order), for a pass that only counts */
__device__ __forceinline__ uint32_t cs_sigmap(int scan, const int16_t (&v)[16])
{
    uint32_t sig[3] = {0, 0, 0};
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int k = 0; k < 16; k++)
            sig[m] |= (uint32_t)(v[cs_raster_of(m, k)] != 0) << k;
    return scan == 0 ? sig[0] : scan == 1 ? sig[1] : sig[2];
}

/* ---- the LCU's transform blocks: block i = 3 * slot + plane ---- */
__device__ __forceinline__ CsTu cs_tu_none(int p)
{
    CsTu T;
    T.coeff_off = 0, T.plane = (uint8_t)p, T.lg = 2, T.scan = 0, T.valid = 0, T.nz = 0, T.sub_base = 0, T.last = -1, T.first_group = 0, T.level_base = 0;
    return T;
}
/* the coded block of plane p in result slot c of unit u (`big`: u is the LCU's lone 64x64 unit, c = 1..4 its four 32x32 transform units); nz: the slot's
 * recorded count.  Returns the block's number of sub-blocks. */
__device__ __forceinline__ uint32_t cs_tu_build(CsTu &T, const SvtAmdLcuCu &u, uint16_t nz, bool big, int c, int p)
{
    const uint32_t size = big ? 32u : u.size, x = big ? 32u * ((c - 1) & 1) : u.x, y = big ? 32u * ((c - 1) >> 1) : u.y;
    const uint32_t ts = p ? (size == 8 ? 4u : size >> 1) : size;
    T.lg = (uint8_t)(31 - __clz((int)ts));
    T.coeff_off = (uint16_t)(p ? 32 * (y >> 1) + (x >> 1) : 64 * y + x);
    T.valid = 1, T.nz = nz;
    if (u.pred_mode == 2 && T.lg <= 3 - (p != 0)) { /* :1347: mode-dependent scan of small intra blocks (chroma follows the luma mode: DM) */
        const int m = u.intra_luma_mode;
        int d = 8 - ((m - 2) & 15);
        d = d < 0 ? -d : d;
        if (d <= 4)
            T.scan = (m & 16) ? 1 : 2;
    }
    return 1u << (2 * (T.lg - 2));
}
/* every thread: block t (t < CS_MAX_TUS, S.tu[t] stored) has nsub sub-blocks; gives the blocks their ranges of the LCU's sub-block index space.  Returns the LCU's
 * number of sub-blocks (the caller sees to it that it is at most CS_MAX_SUBS). */
__device__ __forceinline__ uint32_t cs_place_blocks(CsShared &S, int t, uint32_t nsub)
{
    uint32_t total_subs;
    const uint32_t sub_base = cs_scan256(S, nsub, &total_subs);
    if (t < CS_MAX_TUS && nsub) {
        S.tu[t].sub_base = (uint16_t)sub_base;
        for (uint32_t j = 0; j < nsub; j++)
            S.owner[sub_base + j] = (uint8_t)t;
    }
    __syncthreads();
    return total_subs;
}
/* the 16 values of sub-block q of the LCU into registers: four loads of 4 s16 (x and the plane offsets are multiples of 4 coefficients; the record itself
 * need only be word-aligned).  Returns the block's scan. */
struct __attribute__((aligned(4))) CsRow { uint32_t x, y; };
__device__ __forceinline__ int cs_load_sub(const CsShared &S, const SvtAmdLcuResult *R, uint32_t q, int16_t (&v)[16])
{
    const CsTu T = S.tu[S.owner[q]];
    const uint32_t s = q - T.sub_base;
    uint32_t gy = c_rt.sb[T.lg - 2][s] >> 4, gx = c_rt.sb[T.lg - 2][s] & 15;
    if (T.scan == 1) { const uint32_t tmp = gx; gx = gy, gy = tmp; } /* sub-block scan mirrored for the horizontal scan (:1388) */
    const uint32_t stride = T.plane ? 32 : 64;
    const int16_t *plane = T.plane == 0 ? R->coeff_y : T.plane == 1 ? R->coeff_cb : R->coeff_cr;
    const int16_t *p0 = plane + T.coeff_off + 4 * gy * stride + 4 * gx;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const CsRow w = *(const CsRow *)(p0 + r * stride);
        v[4 * r + 0] = (int16_t)(w.x & 0xFFFF), v[4 * r + 1] = (int16_t)(w.x >> 16);
        v[4 * r + 2] = (int16_t)(w.y & 0xFFFF), v[4 * r + 3] = (int16_t)(w.y >> 16);
    }
    return T.scan;
}
/* every thread, behind a barrier that follows the last write of S.sig / S.cnt: per block the last sub-block and the number of groups and levels, their places in
 * the LCU's lists (S.grp / S.lvl_off of every sub-block, valid behind the caller's next barrier) and block t's record (t < CS_MAX_TUS) */
__device__ __forceinline__ SvtAmdCoeffScanTu cs_finish_blocks(CsShared &S, int t, uint32_t *total_groups, uint32_t *total_levels)
{
    uint32_t ngroups = 0, nlevels = 0;
    if (t < CS_MAX_TUS && S.tu[t].valid) {
        const CsTu T = S.tu[t];
        const uint32_t n = 1u << (2 * (T.lg - 2));
        int last = -1;
        for (uint32_t s = 0; s < n; s++)
            if (S.sig[T.sub_base + s])
                last = (int)s, nlevels += S.cnt[T.sub_base + s];
        S.tu[t].last = (int16_t)last;
        ngroups = (uint32_t)(last + 1);
    }
    const uint32_t first_group = cs_scan256(S, ngroups, total_groups);
    const uint32_t level_base = cs_scan256(S, nlevels, total_levels);
    SvtAmdCoeffScanTu o;
    o.scan_index = 0, o.last_scan_set = -1, o.pos_last = 0, o.last_x = 0, o.last_y = 0, o.dc_only = 0, o.first_group = 0;
    if (t < CS_MAX_TUS) {
        const CsTu T = S.tu[t];
        if (T.valid) {
            const uint32_t n = 1u << (2 * (T.lg - 2));
            const int last = T.last;
            o.first_group = (uint16_t)first_group, o.last_scan_set = (int8_t)last;
            o.dc_only = T.nz == 1 && (S.sig[T.sub_base] & 1); /* :1308 */
            o.scan_index = o.dc_only ? 0 : T.scan;
            uint32_t lv = level_base;
            for (int s = (int)n - 1; s >= 0; s--) { /* coding order: from the last sub-block down */
                S.grp[T.sub_base + s] = (int16_t)(s <= last ? (int)first_group + (last - s) : -1);
                S.lvl_off[T.sub_base + s] = (uint16_t)lv;
                if (s <= last)
                    lv += S.cnt[T.sub_base + s];
            }
            if (last >= 0 && !o.dc_only) {
                const uint32_t pos_last = 31u - (uint32_t)__clz((int)S.sig[T.sub_base + last]); /* :1444 */
                uint32_t ly = 4u * (c_rt.sb[T.lg - 2][last] >> 4), lx = 4u * (c_rt.sb[T.lg - 2][last] & 15);
                const uint32_t pl = T.scan ? c_rt.col4[pos_last] : c_rt.diag4[pos_last];
                ly += pl >> 2, lx += pl & 3;
                if (T.scan) { const uint32_t tmp = lx; lx = ly, ly = tmp; }
                o.pos_last = (uint8_t)pos_last, o.last_x = (uint8_t)lx, o.last_y = (uint8_t)ly;
            }
        }
    }
    return o;
}
#endif
