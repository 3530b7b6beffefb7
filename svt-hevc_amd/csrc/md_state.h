/* md_state.h - the LCU state of the mode-decision kernels (md_kernels.hip): the LCU's mode-decision state in LDS (MdShared: the mode decision's own luma
 * reconstruction - mdLumaReconNeighborArray as a picture plane - with a ring of neighbour samples, the neighbour-array entries of the 4x4 cells, the source block; what only
 * the closed-loop (I picture) / only the inter kernel keeps), the stage clocks of the mode decision of one LCU, and the macros every leaf uses.  Device code: the including
 * unit sets MD_FN for md_logic.h. */
#pragma once
#include "encdec_device.h"
#include "md_logic.h"
/* stage clocks of the mode decision of one LCU, taken by lane 0 behind the barrier that ends the stage.  MD_PROF_ON: `prof_on`, a register copy of "D.prof != null" the
 * functions that use the marks make once per LCU - the descriptor lives in LDS, and fifteen marks per unit each re-reading the pointer were fifteen LDS round trips per unit */
#define MD_PROF_ON prof_on
/* the marks' bodies live in ONE function outside the unit loop: inlined, thirty marks were ~3 KB of instructions strewn over a loop whose code does not fit the
 * instruction cache (a debug facility on the hot path of the product).  q: &M.prof[0]; the fields behind it are laid out as MdShared declares them. */
__device__ __noinline__ void md_prof_mark(unsigned long long *q, int k, int sub)
{
    const unsigned long long c_ = __builtin_readcyclecounter();
    unsigned long long *prof_t = q + 32, *prof_s = q + 33, *prof_d = q + 34;
    const int depth = *reinterpret_cast<const int *>(q + 34 + 128);
    if (sub) {
        q[16 + k] += c_ - *prof_s, prof_d[depth * 32 + 16 + k] += c_ - *prof_s, *prof_s = c_;
    } else {
        q[k] += c_ - *prof_t, prof_d[depth * 32 + k] += c_ - *prof_t, *prof_t = c_, *prof_s = c_;
    }
}
#define MD_PROF(k)                                                          \
    do {                                                                    \
        if (__builtin_expect(MD_PROF_ON, 0) && threadIdx.x == 0)            \
            md_prof_mark(&M.prof[0], k, 0);                                 \
    } while (0)
/* ... and finer marks inside a stage (svt_amd_debug_md_profile_sub): slot k of 16 gets the clocks since the previous mark of either kind */
#define MD_SUB(k)                                                           \
    do {                                                                    \
        if (__builtin_expect(MD_PROF_ON, 0) && threadIdx.x == 0)            \
            md_prof_mark(&M.prof[0], k, 1);                                 \
    } while (0)

/* HASY: the closed-loop decision keeps the mode decision's luma reconstruction of the LCU (+ ring) here; the open-loop one (P / B pictures of this revision) never reads it */
template <bool HASY>
struct MdLocal8T {
    static constexpr int PY = 144, X0 = 16;
    uint8_t y[HASY ? 65 * PY : 16];
    uint32_t info[17 * 36]; /* (cy + 1) * 36 + cx + 1: cy in [-1, 16), cx in [-1, 33] */
    alignas(16) uint8_t src[64 * 64]; /* rows of words: the distortion and residual loops read four samples at a time */
    __device__ __forceinline__ uint8_t *at(int x, int y_) { return &y[(y_ + 1) * PY + X0 + x]; }
    /* neighbour-array entry of the 4x4 cell at luma sample (x, y) relative to the LCU: what lies below the LCU, right of it (from its
     * first row on) or right of the top-right LCU is never written before this LCU */
    __device__ __forceinline__ uint32_t info_at(int x, int y_) const
    {
        const int cx = x >> 2, cy = y_ >> 2;
        if (cy >= 16 || cx >= 32 || (cy >= 0 && cx >= 16))
            return 0xFFFFFFFFu;
        return info[(cy + 1) * 36 + cx + 1];
    }
};

struct MdFl {
    uint32_t nz, d0, d1, bits; /* non-zero levels, sum (coeff - recon)^2, sum coeff^2 over the quantised area, the estimator's bits */
};

/* what only the closed-loop (I picture) / only the inter kernel keeps in LDS */
struct MdClosedLoop {
    alignas(16) uint8_t pred[MD_MAX_BUF][32 * 32];
    int16_t recon_coeff[MD_MAX_BUF][32 * 32];
    uint8_t best_rec[4][64 * 64];
};
#ifdef MD_TRACE
#define MD_PRED_SLOTS 4 /* (the trace buffer needs the room in LDS; a fifth kept candidate is predicted again by the full loop) */
#else
#define MD_PRED_SLOTS 5 /* one motion-estimation candidate + the merge candidates (two or three at the presets' mvMergeSkipModeCount) are evaluated per unit */
#endif
struct MdInterShared {
    /* a wave's chroma prediction of the candidate it works on: the first half of its luma scratch (a wave's tasks follow one another, the luma block is spent by then) */
    __device__ __forceinline__ uint8_t *wpred_c(int wave, int pl) { return wpred[wave] + pl * 1024; }
    MdMvUnit mvu[9 * 18];          /* (cy + 1) * 18 + cx + 1: 8x8 cells, cy in [-1, 8), cx in [-1, 16] */
    SvtAmdMeCuResult me[SVT_AMD_ME_PU_COUNT]; /* the LCU's motion-estimation candidates */
    SvtAmdTmvpLcu tmvp[2];         /* the co-located picture's motion field at this LCU and the one to its right */
    alignas(16) MdCand me_c[4], mg_c[5]; /* the unit's motion-estimation / merge candidates as their list-building waves leave them (wave 0 appends them to the intra candidates) */
    uint32_t nbtab[SVT_AMD_MD_LEAVES][5]; /* per entry of the leaf list, made with the LCU's inputs (off the chain): where its five spatial neighbours A0, A1, B0, B1, B2 lie - index into
                                    * L.info | index into mvu << 10 | (inside what is decided before the unit, not across a tile edge) << 18 */
    uint4 unit_tab[SVT_AMD_MD_LEAVES]; /* per entry of the leaf list: MdStats of its unit (x, y), the unit's index (z): what every thread derives at the top of a unit, made with the LCU's inputs */
    unsigned task_ctr2;            /* ... and of the chroma blocks of the full loop */
    unsigned task_ctr;             /* md_units_inter's fast loop: the next task of the unit's list (the waves draw tasks as they finish: a bi-predicted block costs twice a uni-predicted one) */
    uint2 me_rate[4];              /* ... and the motion-estimation candidates' rate term and fastLumaRate (they depend on the predictors only: derived beside the AMVP lists) */
    int n_me, n_mg;
    alignas(16) uint8_t wpred[4][64 * 64];     /* a wave's prediction of the candidate it works on, pitch = unit size */
    uint8_t cpred[MD_PRED_SLOTS][64 * 64]; /* the fast loop's predictions of the first motion-compensated candidates, kept for the full loop */
    int8_t slot[MD_MAX_CAND];      /* unused (md_units_inter keeps the slots in registers); still here because removing a member moves every LDS offset behind it */
    EpMcScratch<uint8_t> mc[4];
    alignas(16) uint8_t src_c[2][32 * 32];     /* the LCU's chroma source (CHROMA_MODE_FULL candidates; merge / skip decision of the encode pass) */
    /* CHROMA_MODE_FULL LCUs (chroma in both loops of every candidate, EbModeDecisionProcess.c:439-441) */
    alignas(16) uint8_t cpred_c[MD_PRED_SLOTS][2][32 * 32]; /* the chroma predictions beside cpred, pitch = unit size / 2 */
    int16_t refc[2][132];          /* the unit's open-loop chroma intra references (Cb, Cr) in pu_predict's layout */
    uint32_t sadc[MD_MAX_CAND];    /* unused, kept like slot */
    uint32_t sadc2[MD_MAX_CAND][2]; /* Cb and Cr SAD of the fast loop, one owner per entry */
    uint8_t heavyc[MD_MAX_CAND];   /* unused, kept like slot */
    int nheavyc;                   /* unused, kept like slot */
    MdFl flc[MD_MAX_BUF][2][4];    /* the chroma full loop's sums per buffer, plane and transform unit */
    EpRefPlanes refs[2];           /* the reference pictures' plane pointers and geometry beside the LCU (the kernel argument they come from lives in memory as soon as a
                                    * function takes it by reference: a chain of loads per interpolation otherwise) */
    SvtAmdMdInter X;               /* the picture's inter controls beside the LCU: read per unit (a load from HBM each otherwise) */
    EpRefWindows rw;               /* the luma reference samples around the LCU displaced by the 64x64 unit's motion-estimation vectors, per list (encdec_device.h) */
    EpRefWindowsC rwc;             /* ... and, for CHROMA_MODE_FULL LCUs (chroma in both loops of every candidate), the chroma samples around the same position */
    uint8_t ep_kind[SVT_AMD_MD_LEAVES]; /* SVT_AMD_EP_INTER_* of the final tree's inter units */
    uint8_t fin_leaf[SVT_AMD_LCU_MAX_CUS];
    int nfin;
};
template <bool INTER> struct MdVariant { typedef MdClosedLoop type; };
template <> struct MdVariant<true> { typedef MdInterShared type; };

template <bool INTER>
struct MdShared {
    MdLocal8T<!INTER> L;
    MdLcuState S;
    SvtAmdMdLcu lcu;
    SvtAmdOisLcuResult ois;        /* the LCU's open-loop intra search record */
    SvtAmdMdPicture pic;           /* the picture's controls and rate tables: the full costs index the tables by lane-dependent contexts (a load from HBM each otherwise) */
    RateTables rt;                 /* the estimator's scan / context tables (rate_device.h c_rt: 624 B of constant memory read per coefficient position) beside them */
    SvtAmdCabacCost cost;          /* the picture's coefficient-rate tables: read per coefficient in the full loops, so kept beside the LCU instead of in HBM */
    alignas(16) MdCand cand[MD_MAX_CAND];
    unsigned long long costs[MD_MAX_CAND], fast_rate[MD_MAX_CAND];
    uint32_t sad[MD_MAX_CAND];
    uint32_t sadt[MD_MAX_CAND][4]; /* P / B pictures: the fast loop's luma SAD per candidate and tile (one owner per entry; [0] alone for units below 64x64) */
    uint8_t evaluated[MD_MAX_CAND];
    uint8_t heavy[MD_MAX_CAND];    /* the candidates the fast loop has to predict and measure, packed: the waves take them in turn */
    int nheavy;
    MdBuffers B;
    uint8_t types[MD_MAX_BUF], best[MD_MAX_BUF];
    uint32_t ycbf[MD_MAX_BUF];
    MdFl fl[MD_MAX_BUF][4];
    unsigned long long merge_cost[MD_MAX_BUF], skip_cost[MD_MAX_BUF], y_bits[MD_MAX_BUF], y_dist[MD_MAX_BUF][2];
    uint32_t full_dist[MD_MAX_BUF];
    int leaf, cu_idx, ncand, buffer_total, nfull, full_count, max_buffers, lowest, do_recon, exited, last, update, done, best_first, any_intra;
    uint8_t next_step[SVT_AMD_MD_LEAVES + 3]; /* CalculateNextCuIndex's step behind each entry of the leaf list when its unit is not split (md_next_cu_step), made with the LCU's inputs */
    unsigned long long prof[32], prof_t, prof_s;
    unsigned long long prof_d[4][32]; /* the same sums by the depth of the unit they belong to (svt_amd_debug_md_profile_depth) */
    int prof_depth;
    /* (md_prof_mark addresses prof_t .. prof_depth relative to prof[0]) */
    int16_t ref[132], reff[132], border[132];
    typename MdVariant<INTER>::type V;
    int16_t tiles[4][(INTER ? 1 : 2) * TxRegTile<32>::UNIT]; /* a wave's transpose tile (the I picture's inverse transforms run a unit per N lanes: two 32x32 units) */
    int16_t qbuf[4][32 * 32];
};
static_assert(offsetof(MdShared<true>, prof_t) == offsetof(MdShared<true>, prof) + 256 && offsetof(MdShared<true>, prof_s) == offsetof(MdShared<true>, prof) + 264 &&
                  offsetof(MdShared<true>, prof_d) == offsetof(MdShared<true>, prof) + 272 && offsetof(MdShared<true>, prof_depth) == offsetof(MdShared<true>, prof) + 272 + 1024 &&
                  offsetof(MdShared<false>, prof_depth) == offsetof(MdShared<false>, prof) + 272 + 1024,
              "md_prof_mark's view of the profile fields");

#if defined(__HIP_DEVICE_COMPILE__)
#define MD_LDS(ptr) __builtin_assume(__builtin_amdgcn_is_shared((const __attribute__((address_space(0))) void *)(ptr)))
#else
#define MD_LDS(ptr) ((void)0)
#endif
#ifndef MD_LEAF_CALL
#define MD_LEAF_CALL __noinline__ /* the heavy leaves of the unit chain (interpolation, transform unit) as functions: one copy of their code and registers of their own */
#endif
