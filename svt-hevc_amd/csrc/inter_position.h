/* inter_position.h - where a list's motion-compensated block starts in its reference picture: the position clamp of EncodePassInterPrediction
 * (Codec/EbInterPrediction.c:802-812) and the split of the clamped position into integer sample and fraction.  One text for every kernel that addresses a reference
 * window - ep_inter_predict_core, ep_ref_windows_fill, ep_ref_windows_fill_chroma (encdec_device.h), md_predict_tile (md_inter.h) - for the host half of
 * svt_amd_inter_pu_batch (mcp_kernels.hip), and for tools/inter_position_check.c (a plain C program, tests/test_inter_position_cpu.py pins the values).
 * Plain C (with the statement expression gcc and clang both have); the accessors are __host__ __device__ under hipcc. */
#ifndef SVT_AMD_INTER_POSITION_H
#define SVT_AMD_INTER_POSITION_H

#include <stdint.h>

#ifdef __HIPCC__
#define INTER_POS_FN __host__ __device__ static inline
#else
#define INTER_POS_FN static inline
#endif

/* v * 4 for a v of either sign (origin - 71 is negative for a picture padded by less than 71 samples), without a shift of a negative value */
#define INTER_POS_X4(v) ((int)((unsigned)(v) << 2))

/* One component of the position, in quarter luma samples of the padded reference plane: the unit's position `at` (luma samples of the picture) behind the padding
 * `origin`, displaced by the vector `mv` (quarter samples), kept between 71 samples before the picture and 7 samples behind it (`extent` = the picture's width or
 * height).  qx = INTER_POS_CLAMP(abs_x, originX, mv_x, width), qy = INTER_POS_CLAMP(abs_y, originY, mv_y, height).
 * A macro (a statement expression), not a function: the kernels read `origin` and `mv` from memory, and a call would read all of them before the first addition -
 * the same values in another instruction order than the text this replaces (the gate of round 33: the kernels' code stays what it was). */
#define INTER_POS_CLAMP(at, origin, mv, extent)                                                  \
    ({                                                                                           \
        const int q_ = INTER_POS_X4((at) + (origin)) + (mv), lo_ = INTER_POS_X4((origin) - 71);  \
        const int m_ = q_ > lo_ ? q_ : lo_;                                                      \
        const int hi_ = INTER_POS_X4((extent) + (origin) + 7);                                   \
        m_ < hi_ ? m_ : hi_;                                                                     \
    })

/* integer sample and fraction of a component: luma in quarter samples (fraction 0..3), 4:2:0 chroma in eighth samples of the half-size plane (fraction 0..7).
 * The integer part of a negative position rounds down (an arithmetic shift, as in the reference). */
INTER_POS_FN int inter_pos_int(int q, int chroma) { return chroma ? q >> 3 : q >> 2; }
INTER_POS_FN int inter_pos_frac(int q, int chroma) { return chroma ? q & 7 : q & 3; }

/* ---- pictures coded without sub-sample search (useSubpelFlag 0) ----
 * RoundMv (Codec/EbModeDecision.c:200) / RoundMvOnTheFly (Codec/EbInterPrediction.c:46): a vector component to whole samples, (v + 2) & ~3 in int, stored back into 16
 * bits as written - 32766 and 32767 become -32768.  Applied twice it changes nothing more. */
INTER_POS_FN int inter_mv_round(int v) { return (int)(int16_t)(uint16_t)(((unsigned)v + 2u) & ~3u); }
/* ... of both components of a vector packed x | y << 16 (the kernels' form of a vector) */
INTER_POS_FN unsigned inter_mv_round2(unsigned w) { return (((w & 0xFFFFu) + 2u) & 0xFFFCu) | ((((w >> 16) + 2u) & 0xFFFCu) << 16); }

/* The interpolation-free prediction (UniPredIFreeRef8Bit / BiPredIFreeRef8Bit, Codec/EbAvcStyleMcp.c:172 / :321) copies whole samples from a position derived from the clamped
 * one (qx, qy as INTER_POS_CLAMP leaves them): it calls entry 0 of its function table - the copy - whatever the mapped fraction is.
 * Luma: the integer sample plus IntegerPosoffsetTabX / IntegerPosoffsetTabY[fx + 4 fy] (:19-27; FracMappedPosTab* only choose the argument the copy ignores):
 *   X = {0,0,0,0, 0,0,0,0, 0,0,0,1, 0,0,0,0}   Y = {0,0,0,0, 0,0,0,0, 0,0,0,0, 0,1,1,1}   as bit masks (entry f = bit f): selects, not loads. */
#define INTER_IFREE_TAB_X 0x0800u
#define INTER_IFREE_TAB_Y 0xE000u
INTER_POS_FN int inter_ifree_luma_x(int qx, int qy) { return (qx >> 2) + (int)((INTER_IFREE_TAB_X >> ((qx & 3) + ((qy & 3) << 2))) & 1u); }
INTER_POS_FN int inter_ifree_luma_y(int qx, int qy) { return (qy >> 2) + (int)((INTER_IFREE_TAB_Y >> ((qx & 3) + ((qy & 3) << 2))) & 1u); }
/* 4:2:0 chroma: the NEAREST sample of the half-size plane, not the 4-tap filter - pos >> 3, plus one where pos & 7 > 4 (:226-237, :465-492), each direction by itself */
INTER_POS_FN int inter_ifree_chroma(int q) { return (q >> 3) + ((q & 7) > 4); }

#endif
