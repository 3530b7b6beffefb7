/* md_inter.h - the inter prediction of the mode-decision kernels (md_kernels.hip): Inter2Nx2NPuPredictionHevc (Codec/EbInterPrediction.c:468) /
 * Inter2Nx2NPuPredictionInterpolationFree (:57) of one tile of a plane of a candidate by one wave - the position clamp and the window, then ep_mc8_tile
 * (encdec_device.h) - and of a whole plane. */
#pragma once
#include "encdec_device.h"
#include "md_logic.h"
#include "md_lists.h"
#include "md_state.h"

/* a 64-bit value of lane l (wave-uniform l): two v_readlane instead of two trips through the LDS crossbar */
__device__ __forceinline__ unsigned long long md_readlane64(unsigned long long v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

/* a window of `rows` rows of `cpr` 8-byte chunks from a reference plane (the core's clamped addressing at the plane's ends) into the wave's scratch, rows WP apart: the
 * fall-back of md_predict_tile for a window outside the staged samples - one copy of the code for every tile size */
__device__ __noinline__ void md_window_from_plane(const uint8_t *plane, int stride, int last, int base0, int rows, int cpr, int lane, uint8_t *win)
{
    constexpr int WP = EpMcScratch<uint8_t>::WP;
    MD_LDS(win);
    const int nchunk = rows * cpr;
    for (int i0 = 0; i0 < nchunk; i0 += 128) { /* two loads in flight per lane */
        uint2 v[2];
        int at[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int i = i0 + 64 * u + lane;
            at[u] = -1;
            if (i < nchunk) {
                const int j = i / cpr, m = i - j * cpr, idx = base0 + j * stride + m * 8;
                at[u] = j * WP + m * 8;
                if (idx >= 0 && idx + 8 <= last + 1) {
                    __builtin_memcpy(&v[u], plane + idx, 8);
                } else {
                    uint32_t lo = 0, hi = 0;
                    for (int q = 0; q < 4; q++)
                        lo |= (uint32_t)plane[min(max(idx + q, 0), last)] << (8 * q), hi |= (uint32_t)plane[min(max(idx + 4 + q, 0), last)] << (8 * q);
                    v[u] = make_uint2(lo, hi);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (at[u] >= 0)
                *reinterpret_cast<uint2 *>(&win[at[u]]) = v[u];
    }
}
/* Inter2Nx2NPuPredictionHevc (Codec/EbInterPrediction.c:468) of ONE TILE (TN x TN samples: the whole block of a unit up to 32x32 / its chroma block, a quarter of a 64x64
 * unit's luma) of plane p of a candidate, by one wave, both lists: the position clamp and the window, then ep_mc8_tile (encdec_device.h) with the tile size and the tap count decided at compile time -
 * a function per size (the 16x16 and 8x8 blocks most units have need a fraction of the registers of the 32x32 form: no callee-saved register, so no private-segment traffic
 * around the call), everything passed BY VALUE (a candidate passed by reference went through the private segment: a memory round trip of ~1.5 K clocks per call on the unit
 * chain).  mv0 / mv1: x | y << 16.  td: the tile's first sample in the destination, pitch in samples. */
/* IFREE: the picture is coded without sub-sample search (SvtAmdMdInter.use_subpel == 0) - Inter2Nx2NPuPredictionInterpolationFree (Codec/EbInterPrediction.c:57) with
 * roundMvToInteger: the vector goes to whole samples first (RoundMvOnTheFly, :46: what the reference does to a merge candidate's vector, Codec/EbProductCodingLoop.c:2009 /
 * :4239; the candidates of the motion estimation were rounded at their injection and stay what they are), then UniPredIFreeRef8Bit / BiPredIFreeRef8Bit
 * (Codec/EbAvcStyleMcp.c:172 / :321) COPY whole samples - luma from the interpolation-free position, chroma from the NEAREST sample instead of through the 4-tap filter - and
 * average the two lists' copies, (a + b + 1) / 2.  The copy and the average are ep_mc8_tile at the fraction 0, passed as a constant: with the identity taps its two passes
 * reduce to sample s exactly (luma: 64 (64 (s - 128)) + 8192 * 64 + 2048 >> 12 = s; chroma: 64 (64 s) + 2048 >> 12 = s), and BiPredClipping of two such intermediates to
 * ((64 a - 8192) + (64 b - 8192) + 16448) >> 7 = (64 (a + b) + 64) >> 7 = (a + b + 1) >> 1 (chroma: (64 a + 64 b + 64) >> 7, the same).  The window is the filter's
 * (the staged samples, or md_window_from_plane's clamped addressing): the copy reads its middle.  A template parameter: the instances of pictures with sub-sample search
 * hold none of this. */
template <int TN, bool CHROMA, bool IFREE = false>
__device__ MD_LEAF_CALL void md_predict_tile(const EpRefPlanes *refs, int abs_x, int abs_y, int inter_dir, uint32_t mv0, uint32_t mv1, int p, int lane, EpMcScratch<uint8_t> *Mp,
                                             uint8_t *td, int pitch, int tx0, int ty0, const EpRefWindows *RW, const EpRefWindowsC *RWC)
{
    constexpr int WP = EpMcScratch<uint8_t>::WP;
    constexpr int ntaps = CHROMA ? 4 : 8, first = CHROMA ? -1 : -3, rows = TN + ntaps - 1, cpr = (rows + 7) >> 3;
    EpMcScratch<uint8_t> &M = *Mp;
    MD_LDS(Mp), MD_LDS(td), MD_LDS(RW), MD_LDS(RWC), MD_LDS(refs);
    const bool bi = inter_dir == 2;
    bool second = false;
    for (int l = 0; l < 2; l++) {
        if (!(bi || inter_dir == l))
            continue;
        MD_TR(40);
        const EpRefPlanes R = refs[l]; /* one read of the whole record */
        const uint32_t mvw = IFREE ? inter_mv_round2(l ? mv1 : mv0) : (l ? mv1 : mv0);
        const int mvx = (int)(int16_t)(mvw & 0xFFFF), mvy = (int)(int16_t)(mvw >> 16);
        const int qx = INTER_POS_CLAMP(abs_x, R.originX, mvx, R.width), qy = INTER_POS_CLAMP(abs_y, R.originY, mvy, R.height);
        const int ix = (IFREE ? (CHROMA ? inter_ifree_chroma(qx) : inter_ifree_luma_x(qx, qy)) : inter_pos_int(qx, CHROMA)) + tx0;
        const int iy = (IFREE ? (CHROMA ? inter_ifree_chroma(qy) : inter_ifree_luma_y(qx, qy)) : inter_pos_int(qy, CHROMA)) + ty0;
        const int fx = IFREE ? 0 : __builtin_amdgcn_readfirstlane(inter_pos_frac(qx, CHROMA)), fy = IFREE ? 0 : __builtin_amdgcn_readfirstlane(inter_pos_frac(qy, CHROMA));
        MD_TR(41);
        /* where the filter reads the window: a staged one where it lies (EpRefWindows / EpRefWindowsC), any other from the scratch copy the fall-back below makes - ONE
         * instance of the filter per tile size either way (two were ~1 K instructions more per function, in a loop whose code does not fit the instruction cache) */
        /* (the window's place as a byte distance from the scratch copy's: all three live in the workgroup's LDS, 16-byte aligned; an integer, not a choice between pointers) */
        int dbase = 0, doff = 0, dpitch = WP;
        bool staged = false;
        if (!CHROMA) {
            if (RW && RW->valid[l]) {
                const int rx = ix + first - RW->x0[l], ry = iy + first - RW->y0[l];
                if (rx >= 0 && ry >= 0 && rx + rows <= EpRefWindows::P && ry + rows <= EpRefWindows::H)
                    staged = true, dbase = (int)(RW->pix[l] - M.win), doff = ry * EpRefWindows::P + rx, dpitch = EpRefWindows::P;
            }
        } else {
            if (RWC && RWC->valid[l]) {
                const int rx = ix + first - RWC->x0[l], ry = iy + first - RWC->y0[l];
                if (rx >= 0 && ry >= 0 && rx + rows <= EpRefWindowsC::P && ry + rows <= EpRefWindowsC::H)
                    staged = true, dbase = (int)(RWC->pix[l][p - 1] - M.win), doff = ry * EpRefWindowsC::P + rx, dpitch = EpRefWindowsC::P;
            }
        }
        if (__builtin_expect(!staged, 0)) {
            md_window_from_plane((const uint8_t *)R.plane[p], (int)R.stride[CHROMA], R.size[CHROMA] - 1, (iy + first) * (int)R.stride[CHROMA] + ix + first, rows, cpr, lane, M.win);
            EP_WAVE_SYNC();
        }
        MD_TR(42);
        ep_mc8_tile<TN, CHROMA>(M, lane, fx, fy, !bi ? 0 : (second ? 2 : 1), td, pitch, M.win + dbase, doff, dpitch);
        MD_TR(44);
        second = true;
    }
}
/* ... of plane p (0 luma: N x N, 1 / 2 chroma: N/2 x N/2) of a candidate (direction, vectors x | y << 16) into dst with pitch = the block's width; tile_first / tile_step
 * let several waves share the four 32x32 tiles of a 64x64 unit's luma */
template <bool IFREE = false>
__device__ __forceinline__ void md_predict_inter_plane(const EpRefPlanes *refs, int dir, uint32_t mv0, uint32_t mv1, int x0, int y0, int N, int p, int lane, EpMcScratch<uint8_t> &mc,
                                                       uint8_t *dst, int tile_first, int tile_step, const EpRefWindows *rw, const EpRefWindowsC *rwc = nullptr)
{
    const int n = p ? N >> 1 : N, pitch = n;
    if (!p) {
        switch (n) {
        case 64:
            for (int ti = tile_first; ti < 4; ti += tile_step) {
                const int ty0 = (ti >> 1) << 5, tx0 = (ti & 1) << 5;
                md_predict_tile<32, false, IFREE>(refs, x0, y0, dir, mv0, mv1, 0, lane, &mc, dst + ty0 * pitch + tx0, pitch, tx0, ty0, rw, rwc);
            }
            break;
        case 32: md_predict_tile<32, false, IFREE>(refs, x0, y0, dir, mv0, mv1, 0, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        case 16: md_predict_tile<16, false, IFREE>(refs, x0, y0, dir, mv0, mv1, 0, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        default: md_predict_tile<8, false, IFREE>(refs, x0, y0, dir, mv0, mv1, 0, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        }
    } else {
        switch (n) {
        case 32: md_predict_tile<32, true, IFREE>(refs, x0, y0, dir, mv0, mv1, p, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        case 16: md_predict_tile<16, true, IFREE>(refs, x0, y0, dir, mv0, mv1, p, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        case 8: md_predict_tile<8, true, IFREE>(refs, x0, y0, dir, mv0, mv1, p, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        default: md_predict_tile<4, true, IFREE>(refs, x0, y0, dir, mv0, mv1, p, lane, &mc, dst, pitch, 0, 0, rw, rwc); break;
        }
    }
}
template <bool IFREE = false>
__device__ __forceinline__ void md_predict_inter_plane(const EpRefPlanes *refs, const MdCand &c, int x0, int y0, int N, int p, int lane, EpMcScratch<uint8_t> &mc, uint8_t *dst,
                                                       int tile_first, int tile_step, const EpRefWindows *rw, const EpRefWindowsC *rwc = nullptr)
{
    md_predict_inter_plane<IFREE>(refs, (int)c.dir, md_pack_mv(c.mv[0]), md_pack_mv(c.mv[1]), x0, y0, N, p, lane, mc, dst, tile_first, tile_step, rw, rwc);
}
