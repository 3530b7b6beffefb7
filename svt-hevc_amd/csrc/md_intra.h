/* md_intra.h - the intra leaves of the mode-decision kernels (md_kernels.hip): the unit's intra reference by ONE wave - closed loop
 * (GenerateIntraLumaReferenceSamplesMd, Codec/EbProductCodingLoop.c:280-295; Codec/EbIntraPrediction.c:750) and from SOURCE samples (IntraPredictionOl's
 * UpdateNeighborSamplesArrayOL / UpdateChromaNeighborSamplesArrayOL, Codec/EbIntraPrediction.c:4952 / :5065) - and an intra-predicted block by one wave. */
#pragma once
#include "encdec_device.h"
#include "md_logic.h"
#include "md_picture.h"
#include "md_state.h"

/* the unit's intra reference, unfiltered (ref) and filtered (reff), by ONE wave: GenerateLumaIntraReferenceSamplesEncodePass with
 * constrainedIntraFlag 0 / strongIntraSmoothingFlag 1 as GenerateIntraLumaReferenceSamplesMd calls it (Codec/EbProductCodingLoop.c:280-295;
 * Codec/EbIntraPrediction.c:750).  Same scheme as ep_intra_predict_plane (encdec_device.h). */
template <bool INTER>
__device__ __forceinline__ void md_build_refs(MdShared<INTER> &M, const MdStats &st, int lane)
{
    auto &L = M.L;
    const int N = st.size, nb = N >> 2, lgN = st.lg, n = N;
    const bool pic_left = M.lcu.tile_left && st.x == 0, pic_top = M.lcu.tile_top && st.y == 0;
    const bool pic_right = M.lcu.tile_right && ((st.x + N) & 63) == 0;
    const bool bl_ok = md_bottom_left_ok(&st), tr_ok = md_top_right_ok(&st);
    bool a = false;
    if (lane > 4 * nb) {
    } else if (lane < 2 * nb) {
        const int e = (int)(L.info_at(st.x - 1, st.y + 2 * N - 4 - 4 * lane) & 0xFF);
        a = !(e == 0xFE || (!bl_ok && lane < nb) || e == 0xFF || pic_left);
    } else if (lane == 2 * nb) {
        const int e = (int)(L.info_at(st.x - 1, st.y - 1) & 0xFF);
        a = !(e == 0xFE || e == 0xFF || pic_left || pic_top);
    } else {
        const int k = lane - 2 * nb - 1, e = (int)(L.info_at(st.x + 4 * k, st.y - 1) & 0xFF);
        a = !(e == 0xFE || (!tr_ok && k >= nb) || e == 0xFF || pic_top || (pic_right && k >= nb));
    }
    const unsigned long long m = __ballot(a);
    const int firstGroup = m ? __ffsll((long long)m) - 1 : 1 << 30;
    for (int k = lane; k <= 4 * n; k += 64) {
        int v = 128;
        if (firstGroup < (1 << 30)) {
            const int gk = k < 2 * n ? k >> 2 : k == 2 * n ? 2 * nb : 2 * nb + 1 + ((k - 2 * n - 1) >> 2);
            const unsigned long long below = m & ((2ull << gk) - 1ull);
            int src;
            if ((below >> gk) & 1ull) {
                src = k;
            } else if (below) {
                const int sg = 63 - __clzll((long long)below);
                src = sg < 2 * nb ? sg * 4 + 3 : sg == 2 * nb ? 2 * n : 2 * n + 1 + (sg - 2 * nb - 1) * 4 + 3;
            } else {
                src = firstGroup < 2 * nb ? firstGroup * 4 : firstGroup == 2 * nb ? 2 * n : 2 * n + 1 + (firstGroup - 2 * nb - 1) * 4;
            }
            v = src < 2 * n ? (int)*L.at(st.x - 1, st.y + 2 * n - 1 - src) : src == 2 * n ? (int)*L.at(st.x - 1, st.y - 1) : (int)*L.at(st.x + (src - 2 * n - 1), st.y - 1);
        }
        M.border[k] = (int16_t)v;
    }
    EP_WAVE_SYNC();
    const int bl = M.border[0], tlv = M.border[2 * n], tr = M.border[4 * n];
    const bool strong = N >= 32 && abs(bl + tlv - 2 * M.border[n]) < 8 && abs(tlv + tr - 2 * M.border[3 * n]) < 8;
    for (int k = lane; k <= 4 * n; k += 64) {
        const int v = M.border[k];
        int f = v;
        if (strong) {
            if (k > 0 && k < 2 * n)
                f = ((2 * n - k) * bl + k * tlv + n) >> (lgN + 1);
            else if (k > 2 * n && k < 4 * n)
                f = ((2 * n - (k - 2 * n)) * tlv + (k - 2 * n) * tr + n) >> (lgN + 1);
        } else if (k > 0 && k < 4 * n) {
            f = (M.border[k - 1] + 2 * v + M.border[k + 1] + 2) >> 2;
        }
        const int o = k < 2 * n ? 2 * n - 1 - k : k;
        M.ref[o] = (int16_t)v, M.reff[o] = (int16_t)f;
    }
    EP_WAVE_SYNC();
}

/* which reference a luma mode predicts from (intraLumaFilterTable, Codec/EbIntraPrediction.c:60-66) */
__device__ __forceinline__ bool md_mode_filtered(int mode, int lgN)
{
    const int dA = abs(mode - 10), dB = abs(mode - 26), dm = dA < dB ? dA : dB;
    const int thrTab = lgN == 2 ? 35 : lgN == 3 ? 7 : lgN == 4 ? 1 : lgN == 5 ? 0 : 10;
    return dm > thrTab && mode != 1;
}

/* the sum of v over the 64 lanes of a fully active wave, in every lane: data-parallel-primitive adds inside the rows of 16 (quad permutes, half-row and row mirror), the two
 * row broadcasts of gfx9 across them, one v_readlane - no trip through the LDS crossbar (a butterfly of __shfl_xor is six of them in a row) */
__device__ __forceinline__ uint32_t md_wave_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  /* quad_perm [1,0,3,2] */
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  /* quad_perm [2,3,0,1] */
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false); /* row_half_mirror */
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false); /* row_mirror: every lane holds its row's sum */
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); /* row_bcast15 into rows 1 and 3 */
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); /* row_bcast31 into rows 2 and 3 */
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ int md_dc_value(const int16_t *ref, int n, int lgn, int lane)
{
    int dc = lane < n ? ref[lane] + ref[2 * n + 1 + lane] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        dc += __shfl_xor(dc, o);
    return (dc + n) >> (lgn + 1);
}

/* An intra-predicted block of n x n samples by one wave, FOUR samples a lane and step (pu_predict4: a run along the row for the planar, DC and vertical-class modes, down the
 * column for the horizontal-class ones): stored to dst (pitch n) when dst is given, otherwise measured against src (pitch sp) - the lane's part of the SAD is returned.  One
 * copy of the predictor for the eight places the mode decision predicts an intra block (a sample per lane and step there: ~200 issue slots per four samples, ~70 here). */
__device__ MD_LEAF_CALL uint32_t md_intra_block(int mode, int n, int lgn, const int16_t *use, int luma_edge, int lane, const uint8_t *src, int sp, uint8_t *dst)
{
    MD_LDS(use);
    if (src)
        MD_LDS(src);
    if (dst)
        MD_LDS(dst);
    const int dcv = mode == 1 ? md_dc_value(use, n, lgn, lane) : 0;
    const bool hc = pu_horizontal_class(mode);
    uint32_t sad = 0;
    for (int g = lane; g < (n * n) >> 2; g += 64) {
        const int a = 4 * (g & ((n >> 2) - 1)), b = g >> (lgn - 2);
        const int x = hc ? b : a, y = hc ? a : b;
        int o[4];
        pu_predict4(mode, n, lgn, use, x, y, dcv, luma_edge != 0, 255, o);
        if (!hc) {
            const uint32_t w = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
            if (dst)
                *reinterpret_cast<uint32_t *>(&dst[y * n + x]) = w;
            else
                sad = __builtin_amdgcn_sad_u8(w, *reinterpret_cast<const uint32_t *>(&src[y * sp + x]), sad);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (dst)
                    dst[(y + k) * n + x] = (uint8_t)o[k];
                else
                    sad += (uint32_t)abs(o[k] - (int)src[(y + k) * sp + x]);
            }
        }
    }
    return sad;
}

/* IntraPredictionOl's reference of the unit (Codec/EbIntraPrediction.c:4952 UpdateNeighborSamplesArrayOL): SOURCE samples around the unit,
 * mid-grey beyond the picture; no substitution, no smoothing.  By one wave; M.ref in pu_predict's layout. */
template <bool INTER>
__device__ __forceinline__ void md_build_refs_ol(const MdPictureDev &D, MdShared<INTER> &M, const MdStats &st, int x0, int y0, int W, int H, int lane)
{
    const int N = st.size;
    const uint8_t *src = D.src[0] + (size_t)y0 * D.src_pitch[0] + x0;
    for (int k = lane; k <= 4 * N; k += 64) {
        int v = 128;
        if (k < 2 * N) {
            if (x0 != 0 && y0 + k < H)
                v = src[(ptrdiff_t)k * D.src_pitch[0] - 1];
        } else if (k == 2 * N) {
            if (x0 != 0 && y0 != 0)
                v = src[-(ptrdiff_t)D.src_pitch[0] - 1];
        } else {
            const int j = k - 2 * N - 1;
            if (y0 != 0 && x0 + j < W)
                v = src[j - (ptrdiff_t)D.src_pitch[0]];
        }
        M.ref[k] = (int16_t)v;
    }
    EP_WAVE_SYNC();
}

/* IntraPredictionOl's chroma references of the unit (Codec/EbIntraPrediction.c:5065 UpdateChromaNeighborSamplesArrayOL): SOURCE chroma samples around the
 * unit, mid-grey beyond the picture.  By one wave; ref[p] in pu_predict's layout (n = N/2). */
__device__ __forceinline__ void md_build_refs_ol_chroma(const MdPictureDev &D, int16_t (*ref)[132], int N, int x0, int y0, int W, int H, int lane)
{
    const int n = N >> 1, cx = x0 >> 1, cy = y0 >> 1, w = W >> 1, h = H >> 1;
    for (int i = lane; i < 2 * (4 * n + 1); i += 64) {
        const int p = i >= 4 * n + 1, k = p ? i - (4 * n + 1) : i;
        const uint8_t *src = D.src[1 + p] + (size_t)cy * D.src_pitch[1] + cx;
        int v = 128;
        if (k < 2 * n) {
            if (cx != 0 && cy + k < h)
                v = src[(ptrdiff_t)k * D.src_pitch[1] - 1];
        } else if (k == 2 * n) {
            if (cx != 0 && cy != 0)
                v = src[-(ptrdiff_t)D.src_pitch[1] - 1];
        } else {
            const int j = k - 2 * n - 1;
            if (cy != 0 && cx + j < w)
                v = src[j - (ptrdiff_t)D.src_pitch[1]];
        }
        ref[p][k] = (int16_t)v;
    }
    EP_WAVE_SYNC();
}
