/* md_lists.h - the AMVP and merge lists of a unit on registers (GenerateL0L1AmvpMergeLists, Codec/EbAdaptiveMotionVectorPrediction.c:2117-3005; ChooseMVPIdx_V2):
 * what the P / B unit loop md_units_inter (md_units_inter.h) and the test kernel k_md_lists_batch (md_kernels.hip) are built on.  Device code: the including unit sets MD_FN for
 * md_logic.h; MD_NB_ARGS expands to md_rl, which the unit loop defines where it uses the macro. */
#ifndef SVT_AMD_MD_LISTS_H
#define SVT_AMD_MD_LISTS_H
#include "md_logic.h"

/* ---- the motion-vector lists of a unit on REGISTERS (round 6): GenerateL0L1AmvpMergeLists (Codec/EbAdaptiveMotionVectorPrediction.c:2117-3005) as md_logic.h restates it
 * (md_amvp_merge_lists_parts - the text the CPU checker runs and the device tests compare with, reference records on both sides), specialised for what a picture fixes:
 * the target picture of list l IS ref_poc[l], so "the neighbour's vector points to the target picture" is a compare of list indices (+ one flag: both lists hold the same
 * picture), and the scale factor of a spatial neighbour that points to the other list's picture is a constant of the picture - the division of ScaleMV happens once per LCU
 * (MdListConsts), not per neighbour.  The five neighbours arrive in registers (v_readlane), both lists are derived side by side: lane l of the wave works on list l. */
struct MdListConsts {
    int same01;      /* ref_poc[0] == ref_poc[1] */
    int need[2];     /* a vector of the OTHER list's picture has to be scaled to reach list l's picture (td != tb) */
    int scale[2];    /* ... by this factor (ScaleMV :28-52) */
    int bslice;
};
__device__ __forceinline__ int md_scale_factor(int tb, int td) /* ScaleMV's factor; tb, td: int16 differences */
{
    tb = md_clip3(-128, 127, tb), td = md_clip3(-128, 127, td);
    const int16_t temp = (int16_t)((0x4000 + ((td >> 1) < 0 ? -(td >> 1) : (td >> 1))) / td);
    return md_clip3(-4096, 4095, (tb * temp + 32) >> 6);
}
__device__ __forceinline__ MdMv md_scale_by(MdMv v, int scale)
{
    MdMv o;
    o.x = (int16_t)md_clip3(-32768, 32767, (scale * v.x + 127 + (scale * v.x < 0)) >> 8);
    o.y = (int16_t)md_clip3(-32768, 32767, (scale * v.y + 127 + (scale * v.y < 0)) >> 8);
    return o;
}
__device__ __forceinline__ MdListConsts md_list_consts(const SvtAmdMdPicture &P, const SvtAmdMdInter &X)
{
    MdListConsts k;
    k.bslice = P.slice_type == 0;
    k.same01 = X.ref_poc[0] == X.ref_poc[1];
    for (int l = 0; l < 2; l++) {
        const int16_t tb = (int16_t)(X.picture_number - X.ref_poc[l]), td = (int16_t)(X.picture_number - X.ref_poc[1 - l]);
        k.need[l] = td != tb;
        k.scale[l] = td != tb && td != 0 ? md_scale_factor(tb, td) : 0;
    }
    return k;
}
/* GetTemporalMVP_V2 / one list of GetTemporalMVPBPicture_V2 (md_temporal_mvp, md_logic.h) */
__device__ __forceinline__ bool md_temporal_mvp_dev(const SvtAmdMdInter &X, const SvtAmdTmvpLcu *map, MdTmvpPos t, int targetList, MdMv *out)
{
    int colList = X.is_low_delay ? targetList : 1 - X.colocated_pu_ref_list;
    const SvtAmdTmvpLcu *m = &map[t.bottom_right ? t.lcu_offset : 0];
    if (!t.bottom_right && !m->available[t.unit])
        return false;
    const int pd = m->pred_dir[t.unit];
    colList = pd == MD_BI ? colList : pd;
    MdMv v;
    v.x = m->mv[colList][t.unit][0], v.y = m->mv[colList][t.unit][1];
    const int16_t td = (int16_t)(X.colocated_poc - m->ref_poc[colList][t.unit]), tb = (int16_t)(X.picture_number - X.ref_poc[targetList]);
    if (td != tb)
        v = md_scale_by(v, md_scale_factor(tb, td));
    *out = v;
    return true;
}
/* A neighbour's motion as THREE PACKED WORDS (mv[0], mv[1]: x | y << 16; dir | avail << 8) and the lists as words too: every selection below is a select between VALUES.
 * (With MdMvUnit records, `scaled(A0.avail ? A0 : A1)` and `i == 0 ? m[0] : m[1]` are selects between ADDRESSES - the compiler then keeps the records in the private segment:
 * 15 scratch stores per unit and list-building wave and memory-latency loads behind them, 130 MB of HBM writes per 4K picture, profiles/r06_aa.) */
/* ... as fifteen VALUE parameters (an aggregate, however it is indexed, invites the optimiser to turn `b0 ? m0[B0] : m0[B1]` back into a load from a selected address) */
#define MD_NB_PARAMS uint32_t A0m0, uint32_t A0m1, uint32_t A0da, uint32_t A1m0, uint32_t A1m1, uint32_t A1da, uint32_t B0m0, uint32_t B0m1, uint32_t B0da, \
                     uint32_t B1m0, uint32_t B1m1, uint32_t B1da, uint32_t B2m0, uint32_t B2m1, uint32_t B2da
#define MD_NB_ARGS(w0, w1, w2) md_rl(w0, MD_A0), md_rl(w1, MD_A0), md_rl(w2, MD_A0), md_rl(w0, MD_A1), md_rl(w1, MD_A1), md_rl(w2, MD_A1), md_rl(w0, MD_B0), md_rl(w1, MD_B0), \
                               md_rl(w2, MD_B0), md_rl(w0, MD_B1), md_rl(w1, MD_B1), md_rl(w2, MD_B1), md_rl(w0, MD_B2), md_rl(w1, MD_B2), md_rl(w2, MD_B2)
__device__ __forceinline__ uint32_t md_pack_mv(MdMv v) { return (uint32_t)(uint16_t)v.x | ((uint32_t)(uint16_t)v.y << 16); }
__device__ __forceinline__ MdMv md_unpack_mv(uint32_t w)
{
    MdMv v;
    v.x = (int16_t)(w & 0xFFFF), v.y = (int16_t)(w >> 16);
    return v;
}
/* the AMVP candidates of list `list` (a per-lane value): GetSpatialMVPPosAx_V3 / GetNonScalingSpatialMVPPosBx_V3 / GetScalingSpatialMVPPosBx_V3 + the temporal candidate + the
 * zero fill -> c0, c1 (packed), count */
__device__ __forceinline__ int md_amvp_one_list(const MdListConsts &K, const SvtAmdMdInter &X, MD_NB_PARAMS, const SvtAmdTmvpLcu *map, MdTmvpPos tp, int list, uint32_t *c0o, uint32_t *c1o)
{
    const int need = list ? K.need[1] : K.need[0], scale = list ? K.scale[1] : K.scale[0];
    /* non-scaling: the neighbour's vector that points to list `list`'s picture */
    auto nonscale = [&](uint32_t m0, uint32_t m1, uint32_t da, uint32_t *out) -> bool {
        const int dir = (int)(da & 0xFF);
        if (dir == MD_BI) {
            *out = list ? m1 : m0;
            return true;
        }
        const bool ok = dir == list || K.same01;
        if (ok)
            *out = dir ? m1 : m0;
        return ok;
    };
    /* scaling: always available */
    auto scaled = [&](uint32_t m0, uint32_t m1, uint32_t da) -> uint32_t {
        const int dir = (int)(da & 0xFF), l2 = dir == MD_BI ? list : dir;
        uint32_t v = l2 ? m1 : m0;
        if (l2 != list && need)
            v = md_pack_mv(md_scale_by(md_unpack_mv(v), scale));
        return v;
    };
    const bool a0 = (A0da >> 8) & 1, a1 = (A1da >> 8) & 1, b0 = (B0da >> 8) & 1, b1 = (B1da >> 8) & 1, b2 = (B2da >> 8) & 1;
    uint32_t c0 = 0, c1 = 0;
    int num = 0;
    bool ax = false;
    uint32_t v = 0;
    if (a0)
        ax = nonscale(A0m0, A0m1, A0da, &v);
    if (!ax && a1)
        ax = nonscale(A1m0, A1m1, A1da, &v);
    if (!ax && (a0 || a1))
        v = scaled(a0 ? A0m0 : A1m0, a0 ? A0m1 : A1m1, a0 ? A0da : A1da), ax = true;
    if (ax)
        c0 = v, num = 1;
    bool bx = false;
    uint32_t vb = 0;
    if (b0)
        bx = nonscale(B0m0, B0m1, B0da, &vb);
    if (!bx && b1)
        bx = nonscale(B1m0, B1m1, B1da, &vb);
    if (!bx && b2)
        bx = nonscale(B2m0, B2m1, B2da, &vb);
    /* (a vector a failed test left behind is overwritten or never counted, exactly as in the reference's array) */
    if (bx) {
        if (num == 0)
            c0 = vb;
        else
            c1 = vb;
        num++;
    }
    if (!ax && (b0 || b1 || b2)) { /* (ax false: no A neighbour, so at most one candidate so far) */
        const uint32_t vs = scaled(b0 ? B0m0 : b1 ? B1m0 : B2m0, b0 ? B0m1 : b1 ? B1m1 : B2m1,
                                   b0 ? B0da : b1 ? B1da : B2da);
        if (num == 0)
            c0 = vs;
        else
            c1 = vs;
        num++;
    }
    if (num == 2 && c0 == c1)
        num = 1;
    if (map && num < 2) {
        MdMv tv;
        if (md_temporal_mvp_dev(X, map, tp, list, &tv)) {
            if (num == 0)
                c0 = md_pack_mv(tv);
            else
                c1 = md_pack_mv(tv);
            num++;
        }
    }
    if (num < 1 || (num == 1 && (c0 & 0xFFFF) != 0 && (c0 >> 16) != 0)) {
        if (num == 0)
            c0 = 0;
        else
            c1 = 0;
        num++;
    }
    *c0o = c0, *c1o = c1;
    return num;
}
/* ChooseMVPIdx_V2 for one list (md_choose_mvp, md_logic.h): clips the candidate's vector of that list, picks the nearer predictor */
__device__ __forceinline__ void md_choose_mvp_one(const SvtAmdMdPicture &P, uint32_t ox, uint32_t oy, const MdMv a[3], int count, MdMv *mv, uint8_t *idxOut, MdMv *mvp)
{
    md_clip_mv(&P, ox, oy, mv);
    int idx = 0;
    if (count == 2) {
        const uint32_t d0 = (uint32_t)abs(a[0].x - mv->x) + (uint32_t)abs(a[0].y - mv->y), d1 = (uint32_t)abs(a[1].x - mv->x) + (uint32_t)abs(a[1].y - mv->y);
        idx = d0 <= d1 ? 0 : 1;
    } else if (count > 2) {
        return;
    }
    *idxOut = (uint8_t)idx, *mvp = idx ? a[1] : a[0];
}
/* the merge candidates (md_amvp_merge_lists_parts part 4, :2649-2990) as packed words g0[k] / g1[k] / gd[k] (mv[0], mv[1], dir), always totalMerge of them (the zero vectors
 * fill the list).  t0 / t1 / tok: the temporal candidate's two vectors (packed) and whether list 0's exists (derived by the caller, a lane per list) */
struct MdMerge5 {
    uint32_t g0[5], g1[5], gd[5];
};
__device__ __forceinline__ void md_merge_list_regs(const MdListConsts &K, MD_NB_PARAMS, bool have_map, bool tok, uint32_t t0, uint32_t t1, int totalMerge, MdMerge5 &m)
{
    const int bslice = K.bslice;
    int idx = 0;
    auto add = [&](uint32_t dir, uint32_t v0, uint32_t v1) {
        if (idx < totalMerge) { /* (the reference leaves its loop as soon as the list is full) */
#pragma unroll
            for (int k = 0; k < 5; k++)
                if (idx == k)
                    m.g0[k] = v0, m.g1[k] = v1, m.gd[k] = dir;
        }
        idx++;
    };
    auto differs = [&](uint32_t am0, uint32_t am1, uint32_t ada, uint32_t bm0, uint32_t bm1, uint32_t bda) { /* md_mv_differs */
        if (!bslice)
            return am0 != bm0;
        return (ada & 0xFF) != (bda & 0xFF) || am0 != bm0 || am1 != bm1;
    };
    auto dirof = [&](uint32_t da) { return bslice ? (da & 0xFFu) : (uint32_t)MD_L0; };
    const bool a0 = (A0da >> 8) & 1, a1 = (A1da >> 8) & 1, b0 = (B0da >> 8) & 1, b1 = (B1da >> 8) & 1, b2 = (B2da >> 8) & 1;
#pragma unroll
    for (int k = 0; k < 5; k++)
        m.g0[k] = m.g1[k] = m.gd[k] = 0;
    if (a1)
        add(dirof(A1da), A1m0, A1m1);
    if (idx < totalMerge && b1 && (!a1 || differs(B1m0, B1m1, B1da, A1m0, A1m1, A1da)))
        add(dirof(B1da), B1m0, B1m1);
    if (idx < totalMerge && b0 && (!b1 || differs(B0m0, B0m1, B0da, B1m0, B1m1, B1da)))
        add(dirof(B0da), B0m0, B0m1);
    if (idx < totalMerge && a0 && (!a1 || differs(A0m0, A0m1, A0da, A1m0, A1m1, A1da)))
        add(dirof(A0da), A0m0, A0m1);
    if (idx < totalMerge && idx < 4 && b2 && (!a1 || differs(B2m0, B2m1, B2da, A1m0, A1m1, A1da)) && (!b1 || differs(B2m0, B2m1, B2da, B1m0, B1m1, B1da)))
        add(dirof(B2da), B2m0, B2m1);
    if (idx < totalMerge && have_map && tok) {
        if (bslice)
            add(MD_BI, t0, t1);
        else if (idx < 5)
            add(MD_L0, t0, 0u);
    }
    if (idx < totalMerge && bslice) { /* combined bi-predictive candidates: mvMergeCandIndexArrayForFillingUp (:20-23) */
        const int loopEnd = idx * (idx - 1);
        for (int f = 0; idx < totalMerge && f < loopEnd; f++) {
            const int i0 = f == 0 ? 0 : f == 1 ? 1 : f == 2 ? 0 : f == 3 ? 2 : f == 4 ? 1 : f == 5 ? 2 : f == 6 ? 0 : f == 7 ? 3 : f == 8 ? 1 : f == 9 ? 3 : f == 10 ? 2 : 3;
            const int i1 = f == 0 ? 1 : f == 1 ? 0 : f == 2 ? 2 : f == 3 ? 0 : f == 4 ? 2 : f == 5 ? 1 : f == 6 ? 3 : f == 7 ? 0 : f == 8 ? 3 : f == 9 ? 1 : f == 10 ? 3 : 2;
            const uint32_t c0d = i0 == 0 ? m.gd[0] : i0 == 1 ? m.gd[1] : i0 == 2 ? m.gd[2] : m.gd[3], c0v = i0 == 0 ? m.g0[0] : i0 == 1 ? m.g0[1] : i0 == 2 ? m.g0[2] : m.g0[3];
            const uint32_t c1d = i1 == 0 ? m.gd[0] : i1 == 1 ? m.gd[1] : i1 == 2 ? m.gd[2] : m.gd[3], c1v = i1 == 0 ? m.g1[0] : i1 == 1 ? m.g1[1] : i1 == 2 ? m.g1[2] : m.g1[3];
            if (((c0d + 1) & 1) && ((c1d + 1) & 2) && (!K.same01 || c0v != c1v))
                add(MD_BI, c0v, c1v);
        }
    }
    for (int r = 0; r < 5 && idx < totalMerge; r++) /* zero vectors */
        add(bslice ? MD_BI : MD_L0, 0u, 0u);
}

#endif
