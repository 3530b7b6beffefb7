/* md_units_inter.h - the unit loop of P / B pictures of the mode-decision kernels (md_kernels.hip): ModeDecisionLcu's loop over the units of the leaf list
 * (Codec/EbProductCodingLoop.c:4691-5114) - the decisions are those of md_lcu's loop (which I pictures keep): same md_logic.h rules, same leaves, same arithmetic - arranged
 * for the length of a unit's dependency chain on ONE wave. */
#pragma once
#include "encdec_device.h"
#include "md_logic.h"
#include "md_picture.h"
#include "md_lists.h"
#include "md_state.h"
#include "md_intra.h"
#include "md_txfm.h"
#include "md_inter.h"

/* ---- the unit loop of P / B pictures (round 6) ---------------------------------------------------------------------------------------------------------------------------
 * The decisions are those of md_lcu's loop below (which I pictures keep) - same md_logic.h rules, same leaves, same arithmetic - arranged for the one thing that bounds the
 * picture: the length of a unit's dependency chain on ONE wave (a wave issues an instruction every ~4 clocks, an LDS round trip costs ~30 issue slots, a workgroup barrier
 * with a single-lane stage behind it serialises four SIMDs).  Four barriers per unit instead of ten:
 *   A  contexts + intra candidates (wave 0) | AMVP lists + motion-estimation candidates (wave 1) | merge list + merge candidates (wave 2) | intra references (wave 3)
 *   -- barrier --
 *   B  EVERY wave derives the unit's candidate list in its own registers (lane i = candidate i: first fast loop, evaluated flags, the task list as ballot masks) - nothing
 *      to broadcast, no barrier - and runs its share of the fast-loop tasks
 *   -- barrier --
 *   C  EVERY wave: fast costs (lane per candidate), candidate-buffer replay, PreModeDecision - again redundantly, so each wave knows the survivors - then its share of the
 *      full-loop tasks
 *   -- barrier --
 *   D  wave 0: full costs (lane per survivor), ProductFullModeDecision, CheckHighCostPartition, inter-depth decision, neighbour update, next unit
 *   -- barrier --
 * Candidates live in lane registers of every wave (a field of candidate c is a v_readlane away), not in LDS records read field by field. */
__device__ __forceinline__ int md_nth_bit(unsigned long long m, int k) /* index of the k-th set bit (k < popcount) */
{
    for (int i = 0; i < k; i++)
        m &= m - 1;
    return __ffsll((long long)m) - 1;
}
__device__ __forceinline__ uint32_t md_rl(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
union MdCandWords {
    MdCand c;
    uint32_t w[8];
};
static_assert(sizeof(MdCand) == 32, "a candidate is eight words: type | intra_mode | mpm | dist_ready, me_dist, dir | merge_flag | merge_index | mvp_idx[0], mvp_idx[1], mv[0], mv[1], mvp[0], mvp[1]");

/* PROF: whether the stage marks exist at all - the launches of a profiled call (svt_amd_debug_md_profile) take the instance with them, every other launch the one without:
 * thirty tests of a flag per unit and wave, and their branches between the stages, are not on the product's path */
/* CFULL: the LCU is CHROMA_MODE_FULL (chroma in both loops of every candidate) - an instance of the loop per chroma mode, chosen per LCU: the luma-only LCUs' instance carries
 * none of the chroma tasks' code between its stages */
/* IFREE: the picture is coded without sub-sample search - the motion-estimation candidates are rounded to whole samples at their injection, every prediction is
 * md_predict_tile's interpolation-free form (which rounds the merge candidates' vectors on the fly); the candidates, the records and the encode pass keep the merge vectors */
template <bool PROF, bool CFULL, bool IFREE = false>
__device__ __forceinline__ void md_units_inter(const MdPictureDev &D, int lcu, int lcu_x, int lcu_y, MdShared<true> &M)
{
    const bool prof_on = PROF && __builtin_amdgcn_readfirstlane((int)(D.prof != nullptr)) != 0;
    const SvtAmdMdPicture &P = M.pic; /* the rate tables (indexed by contexts): read where they are */
    /* the picture's and the LCU's CONTROLS in registers: a copy of the records' scalar parts, made once per LCU (a control read from LDS is a ~120-clock round trip on
     * a chain whose every stage tests a dozen of them).  Ph / Lh go to the rules that read controls only; the rate tables and the leaf list stay behind P / M.lcu. */
    SvtAmdMdPicture Ph;
    __builtin_memcpy(&Ph, &M.pic, offsetof(SvtAmdMdPicture, rates));
    SvtAmdMdLcu Lh;
    __builtin_memcpy(&Lh.tile_left, &M.lcu.tile_left, sizeof(SvtAmdMdLcu) - offsetof(SvtAmdMdLcu, tile_left));
    Lh.leaf_count = M.lcu.leaf_count;
    /* the wave index as a UNIFORM value (an SGPR): the compiler cannot know that threadIdx.x >> 6 is the same in all lanes of a wave, and makes every `if (wave == ..)` and
     * every task loop a masked vector region otherwise */
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = t & 63;
    auto &L = M.L;
    const int W = (int)Ph.width, H = (int)Ph.height;
    const int lh = min(64, H - lcu_y);
    const SvtAmdOisLcuResult *ois = &M.ois;
    const int pf = md_pf_mode(&Ph);
    /* what the picture and the LCU fix, read once */
    constexpr bool cfull = CFULL; /* CHROMA_MODE_FULL (Lh.chroma_encode_mode == 1): chroma in both loops of every candidate */
    const bool tile_l = Lh.tile_left != 0, tile_t = Lh.tile_top != 0;
    const MdListConsts K = md_list_consts(Ph, M.V.X);
    const uint32_t sfb0 = P.rates.splitFlagBits[0], sfb1 = P.rates.splitFlagBits[1], sfb2 = P.rates.splitFlagBits[2]; /* SplitFlagRate of an unsplit unit, by context */
    const bool tmvp_on = M.V.X.tmvp_enable != 0;
    const unsigned long long lanebit = 1ull << lane, below = lanebit - 1ull;
    /* StopSplitCondition's thresholds of the three depths: what the picture and the LCU fix of md_stop_split (its tables are memory on the device: two dependent loads per
     * call on wave 0's serial stretch of every unit otherwise) */
    const uint32_t ss_thr0 = md_stop_split_threshold(&Ph, &Lh, 0), ss_thr1 = md_stop_split_threshold(&Ph, &Lh, 1), ss_thr2 = md_stop_split_threshold(&Ph, &Lh, 2);
    int cuIdx = M.cu_idx;
    for (;;) {
        MD_TR(10);
        /* ---- the unit (every thread alike) ---- */
        const uint4 ur = M.V.unit_tab[cuIdx]; /* (md_stats of the unit is ~40 instructions and a dependent read of the leaf list: tabulated with the LCU's inputs) */
        const int leaf = (int)ur.z;
        MdStats st;
        {
            const uint32_t w_[2] = {ur.x, ur.y};
            __builtin_memcpy(&st, w_, 8);
        }
        const int N = st.size, lgN = st.lg, x0 = lcu_x + st.x, y0 = lcu_y + st.y;
        const int totalMerge = md_nmm(&Ph, N);
        /* ================= A ================= */
        if (wave == 0) {
            if (lane == 0) {
                M.leaf = leaf;
                if (prof_on)
                    M.prof_depth = st.depth;
                M.S.local[leaf].tested = 1;
                M.S.cu[leaf].split = M.lcu.leaf_split[cuIdx];
                uint32_t l = L.info_at(st.x - 1, st.y), tp = L.info_at(st.x, st.y - 1);
                if ((tile_l && st.x == 0) || (l & 0xFF) == 0xFE)
                    l = 0xFFFFFFFFu;
                if ((tile_t && st.y == 0) || (tp & 0xFF) == 0xFE)
                    tp = 0xFFFFFFFFu;
                MdNeighbors Nb;
                Nb.left_mode = (uint8_t)l, Nb.left_intra = (uint8_t)(l >> 8), Nb.left_depth = (uint8_t)(l >> 16), Nb.left_skip = (uint8_t)(l >> 24);
                Nb.top_mode = (uint8_t)tp, Nb.top_intra = (uint8_t)(tp >> 8), Nb.top_depth = (uint8_t)(tp >> 16), Nb.top_skip = (uint8_t)(tp >> 24);
                md_context_generation(&M.S, leaf, st.y, &Nb);
                M.S.cu[leaf].split = (uint8_t)md_skip_small_cu(&Ph, &Lh, &M.S, leaf, st.depth);
                int ncand = 0;
                if (st.depth != 0 && (st.depth == 3 || !Lh.restrict_intra_global_motion))
                    if (!(Ph.limit_intra && st.x == 0 && st.y == 0))
                        ncand = md_intra_candidates(&Ph, &M.lcu, ois, leaf, &st, M.cand);
                M.ncand = ncand; /* the intra candidates; the other waves' follow */
                M.V.task_ctr = 0, M.V.task_ctr2 = 0;
            }
            MD_TR(11);
            MD_SUB(0);
        } else if (wave < 3) {
            /* the five spatial neighbours (A0, A1, B0, B1, B2; availability as GenerateL0L1AmvpMergeLists derives it, :2256-2340): a lane each, then all five in registers */
            uint32_t w0 = 0, w1 = 0, w2 = 0;
            if (lane < 5) { /* (the mode and the vectors are requested together: one LDS round trip behind the table's) */
                const uint32_t e = M.V.nbtab[cuIdx][lane];
                const uint32_t inf = L.info[e & 1023u];
                const uint32_t *q = reinterpret_cast<const uint32_t *>(&M.V.mvu[(e >> 10) & 255u]);
                const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
                if (((e >> 18) & 1u) && (inf & 0xFF) == MD_INTER)
                    w0 = q0, w1 = q1, w2 = (q2 & 0xFFu) | 0x100u; /* mv[0], mv[1], dir | avail << 8 */
            }
            MD_TR(12);
            const SvtAmdTmvpLcu *map = tmvp_on ? M.V.tmvp : nullptr;
            MdTmvpPos tp;
            tp.bottom_right = 0, tp.lcu_offset = 0, tp.unit = 0, tp.pad = 0;
            if (map)
                tp = md_tmvp_position(&Ph, map, x0, y0, N);
            const int list = lane & 1; /* list-specific work: lane l on list l */
            bool keep = false;
            MdCandWords cw;
            cw.w[0] = MD_INTER, cw.w[1] = cw.w[2] = cw.w[3] = cw.w[4] = cw.w[5] = cw.w[6] = cw.w[7] = 0;
            if (wave == 1) {
                /* both AMVP lists side by side, then Me2Nx2NCandidatesInjection: a lane per motion-estimation candidate */
                /* the unit's motion-estimation record: requested BEFORE the lists are built (it depends on no neighbour), used behind them */
                static_assert(sizeof(SvtAmdMeCuResult) == 24, "six words: vectors, distortions, directions | count");
                const uint32_t *mew = reinterpret_cast<const uint32_t *>(&M.V.me[md_raster_index(&st)]);
                const uint32_t me_v0 = mew[0], me_v1 = mew[1], me_dw = mew[5], me_dist = mew[2 + (lane < 3 ? lane : 0)];
                uint32_t pa0, pa1;
                const int num = md_amvp_one_list(K, M.V.X, MD_NB_ARGS(w0, w1, w2), map, tp, list, &pa0, &pa1);
                MD_TR(13);
                if (lane < 3 && lane < (int)(me_dw >> 24)) {
                    const int dir = (int)((me_dw >> (8 * lane)) & 0xFFu);
                    if (!(dir == MD_BI && Ph.depth_mode == 0 && Lh.lcu_md_mode == 10)) {
                        keep = true;
                        cw.w[0] = MD_INTER | (1u << 24); /* type | dist_ready << 24 */
                        /* RoundMv (Codec/EbModeDecision.c:200, called at :481): all four components, BEFORE the predictor choice below */
                        cw.w[1] = me_dist, cw.w[2] = (uint32_t)dir, cw.w[4] = IFREE ? inter_mv_round2(me_v0) : me_v0, cw.w[5] = IFREE ? inter_mv_round2(me_v1) : me_v1;
                    }
                }
#pragma unroll
                for (int l = 0; l < 2; l++) { /* ChooseMVPIdx_V2 with list l's candidates (lane l holds them) */
                    MdMv al[3];
                    const uint32_t q0 = md_rl(pa0, l), q1 = md_rl(pa1, l);
                    const int cnt = (int)md_rl((uint32_t)num, l);
                    al[0] = md_unpack_mv(q0), al[1] = md_unpack_mv(q1), al[2] = al[1];
                    if (keep && (cw.c.dir == MD_BI || cw.c.dir == l))
                        md_choose_mvp_one(Ph, (uint32_t)x0, (uint32_t)y0, al, cnt, &cw.c.mv[l], &cw.c.mvp_idx[l], &cw.c.mvp[l]);
                }
                if (keep) { /* InterFastCost*sliceOpt's rate of a candidate that is not a merge candidate reads no context of the unit: this wave is not the longest of the four */
                    MdCu none;
                    none.skip_ctx = 0;
                    uint64_t r64 = 0;
                    const uint32_t rt32 = (uint32_t)md_inter_fast_cost_c(&Ph, &st, &none, &cw.c, 0, 0, 0, 1, &r64);
                    M.V.me_rate[__popcll(__ballot(keep) & below)] = make_uint2(rt32, (uint32_t)r64);
                }
            } else {
                /* the temporal candidate's two vectors side by side, the merge list, then ProductMergeSkip2Nx2NCandidatesInjection: a lane per merge candidate */
                MdMv tv;
                tv.x = tv.y = 0;
                bool tok = false;
                if (map && (list == 0 || K.bslice)) {
                    tok = md_temporal_mvp_dev(M.V.X, map, tp, list, &tv);
                    if (!tok)
                        tv.x = tv.y = 0;
                }
                const uint32_t ptv = md_pack_mv(tv), q0 = md_rl(ptv, 0), q1 = md_rl(ptv, 1);
                const bool tok0 = md_rl((uint32_t)tok, 0) != 0;
                MdMerge5 mg;
                md_merge_list_regs(K, MD_NB_ARGS(w0, w1, w2), map != nullptr, tok0, q0, q1, totalMerge, mg);
                MD_TR(13);
                const int k = lane;
                if (k < 5 && k < totalMerge) {
                    const uint32_t c0v = k == 0 ? mg.g0[0] : k == 1 ? mg.g0[1] : k == 2 ? mg.g0[2] : k == 3 ? mg.g0[3] : mg.g0[4];
                    const uint32_t c1v = k == 0 ? mg.g1[0] : k == 1 ? mg.g1[1] : k == 2 ? mg.g1[2] : k == 3 ? mg.g1[3] : mg.g1[4];
                    const uint32_t cd = k == 0 ? mg.gd[0] : k == 1 ? mg.gd[1] : k == 2 ? mg.gd[2] : k == 3 ? mg.gd[3] : mg.gd[4];
                    bool dup = false;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const bool f0 = c0v == mg.g0[j];
                        const bool f1 = cd != MD_L0 && c1v == mg.g1[j];
                        const bool same = cd == MD_L0 ? f0 : (cd == MD_L1 ? f1 : (f0 && f1));
                        dup = dup || (j < k && cd == mg.gd[j] && same);
                    }
                    if (!dup) {
                        keep = true;
                        cw.w[2] = cd | (1u << 8) | ((uint32_t)k << 16); /* dir | merge_flag << 8 | merge_index << 16 */
                        cw.w[4] = c0v, cw.w[5] = c1v;
                    }
                }
            }
            const unsigned long long km = __ballot(keep);
            if (keep) {
                uint4 *dst = reinterpret_cast<uint4 *>(&(wave == 1 ? M.V.me_c : M.V.mg_c)[__popcll(km & below)]);
                dst[0] = make_uint4(cw.w[0], cw.w[1], cw.w[2], cw.w[3]), dst[1] = make_uint4(cw.w[4], cw.w[5], cw.w[6], cw.w[7]);
            }
            if (lane == 0)
                (wave == 1 ? M.V.n_me : M.V.n_mg) = __popcll(km);
            MD_TR(16);
        } else if (st.depth != 0) {
            /* the unit's intra reference from SOURCE samples (IntraPredictionOl; only units below 64x64 have intra candidates) */
            md_build_refs_ol(D, M, st, x0, y0, W, H, lane);
            if (cfull)
                md_build_refs_ol_chroma(D, M.V.refc, N, x0, y0, W, H, lane);
            MD_TR(14);
        }
        MD_SUB(2);
        __syncthreads();
        MD_TR(15);
        MD_SUB(3);
        /* ================= B: the candidate list in the lanes of EVERY wave ================= */
        const int ni = M.ncand, nme = M.V.n_me, nmg = M.V.n_mg, nc = ni + nme + nmg;
        const bool in = lane < nc;
        MdCandWords cw;
        {
            const MdCand *src = lane < ni ? &M.cand[lane] : lane < ni + nme ? &M.V.me_c[lane - ni] : &M.V.mg_c[in ? lane - ni - nme : 0];
            const uint4 a = reinterpret_cast<const uint4 *>(src)[0], b = reinterpret_cast<const uint4 *>(src)[1];
            cw.w[0] = a.x & 0xFF00FFFFu /* mpm = 0: no most-probable-mode search in P / B pictures */, cw.w[1] = a.y, cw.w[2] = a.z, cw.w[3] = a.w, cw.w[4] = b.x, cw.w[5] = b.y, cw.w[6] = b.z,
            cw.w[7] = b.w;
        }
        const MdCand &c = cw.c;
        const int ctype = in ? c.type : 0;
        const MdCu cuv = M.S.cu[leaf]; /* the unit's contexts (wave 0 left them before the barrier) */
        int bufferTotal = md_nfl(&Ph, &Lh, N);
        bufferTotal = nc < bufferTotal ? nc : bufferTotal;
        const int width = st.depth == 0 ? 5 : 8, max_buffers = bufferTotal + 1 < width ? bufferTotal + 1 : width;
        const bool any_intra = ni != 0;
        /* the first fast loop (EbProductCodingLoop.c:1948-1988): the best of the candidates whose distortion the open-loop stages left; the reference walks from the last
         * candidate down with <=: the LOWEST index among equal costs */
        /* A candidate's fast cost is (distortion terms) + (lambda * rate + 2^22 >> 23), and the RATE is known before any distortion is: the rules of md_logic.h, called once
         * per candidate with zero distortion, return exactly that rate term (and fastLumaRate).  Fast costs stay below 2^31 (SAD of at most 64 x 64 8-bit samples << 8, a
         * chroma term of the same size, a rate term below 2^18): everything downstream - the first fast loop here, the fast costs, the candidate buffers and PreModeDecision
         * behind the second barrier - runs on 32-bit values. */
        unsigned long long rate = 0;
        uint32_t rterm = 0;
        if (in) {
            if (lane >= ni && lane < ni + nme) { /* (derived beside the AMVP lists) */
                const uint2 pr = M.V.me_rate[lane - ni];
                rterm = pr.x, rate = pr.y;
            } else {
                rterm = (uint32_t)(c.type == MD_INTER ? md_inter_fast_cost_c(&Ph, &st, &cuv, &c, 0, 0, 0, 1, (uint64_t *)&rate)
                                                      : md_intra_fast_cost_pslice_c(&Ph, &st, &cuv, c.intra_mode, 0, 0, 0, (uint64_t *)&rate));
            }
        }
        int bestFirst = -1;
        {
            const bool ready = in && c.dist_ready;
            const uint32_t cost = ready ? (c.me_dist << 8) + rterm : 0xFFFFFFFFu;
            uint32_t m = 0xFFFFFFFFu;
            unsigned long long rm = __ballot(ready);
            while (rm) {
                const int l = __ffsll((long long)rm) - 1;
                rm &= rm - 1;
                const uint32_t v = md_rl(cost, l);
                if (bestFirst < 0 || v < m)
                    m = v, bestFirst = l;
            }
        }
        int evl = (int)(in && (!c.dist_ready || lane == bestFirst));
        if (evl && lane == bestFirst && c.type == MD_INTRA)
            evl = 3; /* the open-loop distortion stands, no luma prediction (:1660, :2042) */
        /* what the fast loop has to predict + measure: the evaluated candidates except the open-loop intra candidate whose distortion stands (:2042) */
        const bool heavy = in && evl && !(lane == bestFirst && c.type == MD_INTRA);
        const unsigned long long hm = __ballot(heavy);
        const bool hc = in && evl && cfull; /* CHROMA_MODE_FULL: the chroma pair of EVERY evaluated candidate */
        const unsigned long long cm = __ballot(hc);
        const unsigned long long qm = __ballot(evl && c.type == MD_INTER); /* the first MD_PRED_SLOTS inter candidates the loop evaluates keep their prediction for the full loop */
        const int qrank = __popcll(qm & below);
        const int slot = (in && evl && c.type == MD_INTER && qrank < MD_PRED_SLOTS) ? qrank : -1;
        if (wave == 0 && in && lane >= ni) { /* the list as one array (wave 0's full costs read a survivor's record from it) */
            uint4 *dst = reinterpret_cast<uint4 *>(&M.cand[lane]);
            dst[0] = make_uint4(cw.w[0], cw.w[1], cw.w[2], cw.w[3]), dst[1] = make_uint4(cw.w[4], cw.w[5], cw.w[6], cw.w[7]);
        }
        MD_TR(18);
        MD_SUB(6);
        MD_PROF(1);
        MD_PROF(2);
        if (prof_on && t == 0)
            M.prof[13] += (unsigned long long)nc, M.prof[14] += 1, M.prof_d[M.prof_depth][13] += (unsigned long long)nc, M.prof_d[M.prof_depth][14] += 1;
        /* ---- fast loop (ProductPerformFastLoop's second loop): ONE list of tasks = (candidate, plane, tile) dealt to the four waves ---- */
        const bool tiled64 = N == 64 && !any_intra;
        {
            const int nheavy = __popcll(hm), nhc = __popcll(cm);
            const int nl = tiled64 ? nheavy * 4 : nheavy, ntask = nl + 2 * nhc;
            /* up to four tasks: a wave each; more (CHROMA_MODE_FULL LCUs: eight to twelve): the waves DRAW them from a counter as they finish - the tasks differ by a factor of
             * four (a bi-predicted luma block against a uni-predicted 4x4 chroma block), dealt round-robin the slowest wave set the stage's time */
            const bool draw = ntask > 4;
            for (int tk = wave;;) {
                if (draw) {
                    unsigned got = 0;
                    if (lane == 0)
                        got = atomicAdd(&M.V.task_ctr, 1u);
                    tk = (int)md_rl(got, 0);
                }
                if (tk >= ntask)
                    break;
                MD_TR(20);
                const bool luma = tk < nl;
                /* drawn tasks run from the LAST candidate to the first: the list holds the intra candidates first, and their blocks are the short tasks - the long ones
                 * (motion-compensated, two lists) start first, the short ones fill the waves' tails */
                const int kq = luma ? (tiled64 ? tk >> 2 : tk) : (tk - nl) >> 1, ti = luma ? (tiled64 ? tk & 3 : 0) : 0, pl = luma ? 0 : 1 + ((tk - nl) & 1);
                const int k = draw ? (luma ? nheavy : nhc) - 1 - kq : kq;
                const int ci = md_nth_bit(luma ? hm : cm, k);
                const uint32_t cw0 = md_rl(cw.w[0], ci), cw2 = md_rl(cw.w[2], ci);
                uint32_t sad = 0;
                if ((cw0 & 0xFF) == MD_INTER) {
                    const int sl = (int)md_rl((uint32_t)slot, ci), n = luma ? N : N >> 1, lgn = luma ? lgN : lgN - 1;
                    uint8_t *pr = luma ? (sl >= 0 ? M.V.cpred[sl] : M.V.wpred[wave]) : (sl >= 0 ? M.V.cpred_c[sl][pl - 1] : M.V.wpred_c(wave, pl - 1));
                    MD_TR(21);
                    md_predict_inter_plane<IFREE>(M.V.refs, (int)(cw2 & 0xFF), md_rl(cw.w[4], ci), md_rl(cw.w[5], ci), x0, y0, N, pl, lane, M.V.mc[wave], pr, tiled64 && luma ? ti : 0,
                                           tiled64 && luma ? 4 : 1, &M.V.rw, &M.V.rwc);
                    MD_TR(22);
                    MD_SUB(7);
                    if (luma && tiled64) {
                        const int ty0 = (ti >> 1) << 5, tx0 = (ti & 1) << 5;
                        for (int e = 4 * lane; e < 32 * 32; e += 256) { /* v_sad_u8: four samples a word */
                            const int y = ty0 + (e >> 5), x = tx0 + (e & 31);
                            sad = __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t *>(&pr[y * 64 + x]), *reinterpret_cast<const uint32_t *>(&L.src[(st.y + y) * 64 + st.x + x]), sad);
                        }
                    } else if (luma) {
                        for (int e = 4 * lane; e < N * N; e += 256)
                            sad = __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t *>(&pr[e]), *reinterpret_cast<const uint32_t *>(&L.src[(st.y + (e >> lgN)) * 64 + st.x + (e & (N - 1))]), sad);
                    } else { /* chroma blocks are 4 .. 32 samples wide: rows of words */
                        const uint8_t *sc = &M.V.src_c[pl - 1][(st.y >> 1) * 32 + (st.x >> 1)];
                        for (int e = 4 * lane; e < n * n; e += 256)
                            sad = __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t *>(&pr[e]), *reinterpret_cast<const uint32_t *>(&sc[(e >> lgn) * 32 + (e & (n - 1))]), sad);
                    }
                } else if (luma) {
                    sad = md_intra_block((int)((cw0 >> 8) & 0xFF), N, lgN, M.ref, 1, lane, &L.src[st.y * 64 + st.x], 64, nullptr);
                } else { /* IntraPredictionOl's chroma pair: the chroma mode is always DM (Codec/EbIntraPrediction.c:5530) */
                    sad = md_intra_block((int)((cw0 >> 8) & 0xFF), N >> 1, lgN - 1, M.V.refc[pl - 1], 0, lane, &M.V.src_c[pl - 1][(st.y >> 1) * 32 + (st.x >> 1)], 32, nullptr);
                }
                sad = md_wave_sum(sad);
                MD_TR(23);
                MD_SUB(8);
                if (lane == 0) { /* every (candidate, plane, tile) has ONE owner: plain stores, nothing to initialise */
                    if (luma)
                        M.sadt[ci][ti] = sad;
                    else
                        M.V.sadc2[ci][pl - 1] = sad;
                }
                MD_TR(24);
                if (!draw)
                    break; /* (at most four tasks: this wave's one is done) */
            }
        }
        __syncthreads();
        MD_TR(25);
        MD_PROF(3);
        /* ================= C: fast costs (a lane per candidate), candidate buffers (a lane per buffer), PreModeDecision - in every wave ================= */
        uint32_t cst = 0xFFFFFFFFu; /* (a candidate the loop does not evaluate: the all-ones cost of an unused buffer) */
        if (in && evl) {
            uint32_t dist, distc = 0;
            if (heavy)
                dist = tiled64 ? M.sadt[lane][0] + M.sadt[lane][1] + M.sadt[lane][2] + M.sadt[lane][3] : M.sadt[lane][0];
            else
                dist = c.me_dist;
            /* md_inter_fast_cost_c / md_intra_fast_cost_pslice_c (md_logic.h) with the rate term of the first barrier's side */
            if (cfull) { /* the chroma pair's SAD with the noise-class rule (:2079-2094) */
                distc = (uint32_t)md_fast_chroma_noise_rule(&Lh, N, &c, (uint64_t)M.V.sadc2[lane][0] + M.V.sadc2[lane][1]);
                if (c.type == MD_INTER && c.merge_flag && Lh.cmplx_noise)
                    cst = ((dist + distc) << 8) + rterm; /* weightChromaDistortion == 0: a merge candidate's chroma SAD is added unweighted */
                else
                    cst = (dist << 8) + (uint32_t)md_weighted_chroma(distc, M.V.X.chroma_weight) + rterm;
            } else {
                cst = (dist << 8) + rterm;
            }
        } else {
            rate = 0; /* fastLumaRate of a candidate the loop does not evaluate (the reference never computes it) */
        }
        MD_TR(26);
        MD_SUB(9);
        /* md_fast_loop_buffers (md_logic.h; ProductPerformFastLoop's second loop, :1990-2179) with the buffers in lanes 0..7: the candidates arrive from the last to the
         * first, each goes into the buffer with the highest cost (an unused one first) = the FIRST buffer holding the maximum over [0, maxBuffers) */
        uint32_t bcost = 0xFFFFFFFFu;
        int bcand = -1, bpred = -1, evcount = 0;
        {
            int highest = 0;
            const int maxb = max_buffers < 2 ? 2 : max_buffers;
            const bool inb = lane < maxb;
            for (int idx = nc - 1; idx >= 0; idx--) {
                const uint32_t cv = md_rl(cst, idx);
                const int ev = __builtin_amdgcn_readlane(evl, idx);
                if (lane == highest) {
                    bcand = idx;
                    if (ev) {
                        bcost = cv;
                        if (!(ev & 2))
                            bpred = idx;
                    }
                }
                evcount += ev != 0;
                if (idx) { /* the first of lanes [0, maxb) holding their maximum: three DPP steps over the eight lanes, one ballot */
                    static_assert(MD_MAX_BUF == 8, "the buffers are the first eight lanes of a row");
                    const uint32_t v = inb ? bcost : 0u;
                    uint32_t m = v;
                    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, false));  /* quad_perm [1,0,3,2] */
                    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false));  /* quad_perm [2,3,0,1] */
                    m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, false)); /* row_half_mirror */
                    highest = __ffsll((long long)__ballot(inb && bcost == md_rl(m, 0))) - 1;
                }
            }
        }
        MD_TR(27);
        MD_SUB(10);
        /* PreModeDecision (md_pre_mode_decision, md_logic.h; Codec/EbModeDecision.c:300-383) on uniform values: the buffers' costs by v_readlane, the order as nibbles of a word */
        uint32_t best = 0; /* best[f] = (best >> 4 f) & 15 */
        int full_count, nfull;
        /* lane b: the type of buffer b's candidate.  (The shuffle runs in EVERY lane: a lane that sits the instruction out returns zero to whoever reads it - and the
         * candidates beyond the buffer count live in exactly the lanes that hold no buffer.) */
        const int btype_any = __shfl(ctype, bcand < 0 ? 0 : bcand), btype = bcand >= 0 ? btype_any : 0;
        {
            int bt = evcount < bufferTotal ? evcount : bufferTotal;
            const int same = evcount == bt, count = same ? bt : max_buffers;
            const int fullRecon = same ? (count < 1 ? 1 : count) : (count - 1 < 1 ? 1 : count - 1);
            if (count > 1) {
                int skipIdx = -1;
                if (!same) {
                    uint32_t hcost = md_rl(bcost, 0);
                    skipIdx = 0;
                    for (int i = 1; i < count; i++) {
                        const uint32_t v = md_rl(bcost, i);
                        if (v >= hcost)
                            hcost = v, skipIdx = i;
                    }
                }
                int k = 0;
                for (int i = 0; i < count; i++)
                    if (i != skipIdx)
                        best |= (uint32_t)i << (4 * k++);
            }
            const unsigned long long interm = __ballot(btype == MD_INTER) & 0xFFull, intram = __ballot(btype == MD_INTRA) & 0xFFull;
            for (int i = 0; i < fullRecon - 1; i++) /* inter candidates first */
                for (int j = i + 1; j < fullRecon; j++) {
                    const uint32_t bi = (best >> (4 * i)) & 15u, bj = (best >> (4 * j)) & 15u;
                    if (((intram >> bi) & 1ull) && ((interm >> bj) & 1ull))
                        best = (best & ~((15u << (4 * i)) | (15u << (4 * j)))) | (bj << (4 * i)) | (bi << (4 * j));
                }
            full_count = fullRecon;
            nfull = full_count < bt ? full_count : bt;
        }
        MD_TR(28);
        MD_PROF(4);
        /* ---- full loop: a wave per surviving candidate (PerformFullLoop, :4351) ---- */
        /* a 64x64 unit has four 32x32 transform units per candidate: a wave per (candidate, transform unit).  The candidates of a 64x64 unit are motion-compensated. */
        const bool split64 = N == 64 && nfull <= 4 && !any_intra;
        bool fresh64 = false;
        auto buf_cand = [&](int b) { return __builtin_amdgcn_readlane(bcand, b); };
        auto buf_pred = [&](int b) { return __builtin_amdgcn_readlane(bpred, b); };
        auto kept_pred = [&](int pci) { return (int)md_rl((uint32_t)slot, pci) >= 0 && __builtin_amdgcn_readlane(evl, pci) != 0; };
        if (split64) {
            for (int f = 0; f < nfull; f++) {
                const int b = (int)((best >> (4 * f)) & 15u), ci = buf_cand(b), pci = buf_pred(b) < 0 ? ci : buf_pred(b);
                if (!kept_pred(pci)) {
                    fresh64 = true;
                    if (wave == f)
                        md_predict_inter_plane<IFREE>(M.V.refs, (int)(md_rl(cw.w[2], pci) & 0xFF), md_rl(cw.w[4], pci), md_rl(cw.w[5], pci), x0, y0, N, 0, lane, M.V.mc[wave], M.V.wpred[f], 0, 1,
                                               &M.V.rw, &M.V.rwc);
                }
            }
            if (fresh64)
                __syncthreads();
            for (int f = 0; f < nfull; f++) {
                const int b = (int)((best >> (4 * f)) & 15u), ci = buf_cand(b), pci = buf_pred(b) < 0 ? ci : buf_pred(b);
                const uint8_t *pred = kept_pred(pci) ? M.V.cpred[(int)md_rl((uint32_t)slot, pci)] : M.V.wpred[f];
                const int tu = wave, off = ((tu & 1) << 5) + ((tu >> 1) << 5) * 64;
                const uint32_t c0 = md_rl(cw.w[0], ci);
                const MdFl o = md_full_loop_unit<32>(lane, &L.src[st.y * 64 + st.x] + off, 64, pred + off, 64, nullptr, M.tiles[wave], M.qbuf[wave], Ph.qp, Ph.slice_type, M.cost,
                                                     (int)(c0 & 0xFF), (int)((c0 >> 8) & 0xFF), 0, pf, M.rt);
                if (lane == 0)
                    M.fl[b][tu] = o;
                EP_WAVE_SYNC();
            }
        }
        for (int f = wave; f < nfull && !split64; f += 4) {
            MD_TR(30);
            const int b = (int)((best >> (4 * f)) & 15u), ci = buf_cand(b);
            const uint32_t c0 = md_rl(cw.w[0], ci);
            const int cdtype = (int)(c0 & 0xFF), cdmode = (int)((c0 >> 8) & 0xFF);
            /* the buffer's luma prediction: the candidate the fast loop predicted there, or - predictionIsReadyLuma == 0 - a fresh one */
            const bool fresh = ci == bestFirst && cdtype == MD_INTRA && __builtin_amdgcn_readlane(evl, ci) != 0;
            const int pci = (fresh || buf_pred(b) < 0) ? ci : buf_pred(b);
            const uint32_t p0 = md_rl(cw.w[0], pci);
            uint8_t *pred = M.V.wpred[wave];
            if ((p0 & 0xFF) == MD_INTER) {
                if (kept_pred(pci))
                    pred = M.V.cpred[(int)md_rl((uint32_t)slot, pci)]; /* the fast loop's prediction of this candidate is still there */
                else
                    md_predict_inter_plane<IFREE>(M.V.refs, (int)(md_rl(cw.w[2], pci) & 0xFF), md_rl(cw.w[4], pci), md_rl(cw.w[5], pci), x0, y0, N, 0, lane, M.V.mc[wave], pred, 0, 1, &M.V.rw, &M.V.rwc);
            } else {
                md_intra_block((int)((p0 >> 8) & 0xFF), N, lgN, M.ref, 1, lane, nullptr, 0, pred);
                EP_WAVE_SYNC();
            }
            MD_TR(31);
            MD_SUB(12);
            md_full_loop_cand(lane, N, &L.src[st.y * 64 + st.x], pred, N, nullptr, M.tiles[wave], M.qbuf[wave], P, M.cost, M.rt, cdtype, cdmode, pf, M.fl[b]);
            MD_TR(32);
            MD_SUB(13);
        }
        /* CHROMA_MODE_FULL (PerformFullLoop :4443-4560): the chroma pair of every survivor - ChromaPrediction (the candidate's OWN prediction: the fast loop's when it
         * evaluated the candidate, a fresh one otherwise), FullLoop_R + CuFullDistortionFastTuMode_R - as tasks (survivor, plane) on the waves the luma units left idle */
        if (cfull) {
            if (fresh64) /* every wave is done with the fresh luma predictions in the waves' scratch before a chroma block lands there */
                __syncthreads();
            const int Cn = N >> 1, lgc = lgN - 1, Tc = N == 64 ? 16 : Cn, ntu = N == 64 ? 4 : 1;
            /* the waves DRAW the chroma tasks as they get free: a luma unit with levels to price takes twice the time of one without, a wave without a luma unit starts at
             * once - no fixed assignment fits.  A task = (survivor, plane); the 8x8 chroma pair of a 16x16 unit's survivor is ONE task on the matrix cores (md_chroma_pair8). */
            const bool pair8 = N == 16 && !s_md_force_bfly;
            const int ntk = pair8 ? nfull : 2 * nfull;
            for (;;) {
                unsigned got = 0;
                if (lane == 0)
                    got = atomicAdd(&M.V.task_ctr2, 1u);
                const int tk = (int)md_rl(got, 0);
                if (tk >= ntk)
                    break;
                const int f = pair8 ? tk : tk >> 1, pl0 = pair8 ? 0 : tk & 1, pl1 = pair8 ? 2 : pl0 + 1, b = (int)((best >> (4 * f)) & 15u), ci = buf_cand(b);
                const uint32_t c0 = md_rl(cw.w[0], ci);
                const int cdtype = (int)(c0 & 0xFF), cdmode = (int)((c0 >> 8) & 0xFF);
                const uint8_t *pred; /* plane 0's block; plane 1's 1024 bytes behind */
                if (cdtype == MD_INTER && kept_pred(ci)) {
                    pred = M.V.cpred_c[(int)md_rl((uint32_t)slot, ci)][0];
                } else {
                    uint8_t *pw0 = M.V.wpred_c(wave, 0);
                    for (int pl = pl0; pl < pl1; pl++) {
                        uint8_t *pw = pw0 + pl * 1024;
                        if (cdtype == MD_INTER) {
                            md_predict_inter_plane<IFREE>(M.V.refs, (int)(md_rl(cw.w[2], ci) & 0xFF), md_rl(cw.w[4], ci), md_rl(cw.w[5], ci), x0, y0, N, 1 + pl, lane, M.V.mc[wave], pw, 0, 1, &M.V.rw,
                                                   &M.V.rwc);
                        } else {
                            md_intra_block(cdmode, Cn, lgc, M.V.refc[pl], 0, lane, nullptr, 0, pw);
                            EP_WAVE_SYNC();
                        }
                    }
                    pred = pw0;
                }
                if (pair8) {
                    md_chroma_pair8(lane, &M.V.src_c[0][(st.y >> 1) * 32 + (st.x >> 1)], pred, M.qbuf[wave], (int)P.chroma_qp, (int)P.slice_type, M.cost, cdtype, cdmode, pf, M.rt,
                                    &M.V.flc[b][0][0]);
                    continue;
                }
                const int pl = pl0;
                for (int tu = 0; tu < ntu; tu++) {
                    const int ox = ntu == 1 ? 0 : (tu & 1) << 4, oy = ntu == 1 ? 0 : (tu >> 1) << 4;
                    uint32_t nz;
                    unsigned long long d[2], bt;
                    md_chroma_tu(lane, Tc, &M.V.src_c[pl][((st.y >> 1) + oy) * 32 + (st.x >> 1) + ox], pred + pl * 1024 + oy * Cn + ox, Cn, M.tiles[wave], M.qbuf[wave], P, M.cost, M.rt,
                                 cdtype, cdmode, 1 + pl, pf, &nz, d, &bt);
                    if (lane == 0) {
                        MdFl o;
                        o.nz = nz, o.d0 = (uint32_t)d[0], o.d1 = (uint32_t)d[1], o.bits = (uint32_t)bt;
                        M.V.flc[b][pl][tu] = o;
                    }
                }
            }
        }
        MD_TR(33);
        __syncthreads();
        MD_TR(34);
        MD_PROF(5);
        /* ================= D (wave 0): TuCalcCostLuma + the full cost of every survivor (a lane each), ProductFullModeDecision, the depth decisions, the neighbour update ================= */
        if (wave == 0) {
            const bool have = lane < nfull;
            const int b = (int)((best >> (4 * (have ? lane : 0))) & 15u);
            const int ci = __shfl(bcand, b);
            uint32_t ycbf = 0;
            unsigned long long bits = 0, dist[2] = {0, 0}, full = 0;
            uint64_t mc = 0, sc = 0;
            const unsigned long long frate = __shfl(rate, have ? ci : 0); /* fastLumaRate of the survivor's candidate */
            MdCandWords sv; /* the survivor's candidate record */
            {
                const uint4 a = reinterpret_cast<const uint4 *>(&M.cand[have ? ci : 0])[0], bq = reinterpret_cast<const uint4 *>(&M.cand[have ? ci : 0])[1];
                sv.w[0] = a.x, sv.w[1] = a.y, sv.w[2] = a.z, sv.w[3] = a.w, sv.w[4] = bq.x, sv.w[5] = bq.y, sv.w[6] = bq.z, sv.w[7] = bq.w;
            }
            const int svtype = have ? sv.c.type : 0;
            if (have) {
                const MdCand &cs = sv.c;
                if (N == 64) {
                    for (int tu = 0; tu < 4; tu++)
                        md_tu_calc_cost(P, M.fl[b][tu], cs.type, 64, 32, tu + 1, &ycbf, &bits, dist);
                } else {
                    md_tu_calc_cost(P, M.fl[b][0], cs.type, N, N, 0, &ycbf, &bits, dist);
                }
                bits = md_pf_coeff_bits(pf, Ph.qp, bits); /* (CHROMA_MODE_BEST and CHROMA_MODE_FULL LCUs: the only ones md_lcu_supported admits) */
                if (cfull) { /* InterFullCost / MergeSkipFullCost / IntraFullCostPslice: the chroma loop's sums join the luma ones */
                    const int ntu = N == 64 ? 4 : 1;
                    uint32_t cbf[2] = {0, 0};
                    uint64_t cbits[2] = {0, 0}, cdist[2][2] = {{0, 0}, {0, 0}};
                    for (int pl = 0; pl < 2; pl++)
                        for (int tu = 0; tu < ntu; tu++) {
                            const MdFl o = M.V.flc[b][pl][tu];
                            cbf[pl] |= (uint32_t)(o.nz != 0) << (ntu == 1 ? 0 : tu + 1);
                            cbits[pl] += o.bits, cdist[pl][0] += o.d0, cdist[pl][1] += o.d1;
                        }
                    const uint64_t yd[2] = {dist[0], dist[1]};
                    if (cs.type == MD_INTER)
                        full = md_inter_full_cost(&P, M.V.X.chroma_weight, &cuv, &cs, N, ycbf, cbf, frate, yd, cdist, bits, cbits, &mc, &sc);
                    else
                        full = md_intra_full_cost_pslice(&P, M.V.X.chroma_weight, N, ycbf, cbf, frate, dist[0], cdist, bits, cbits);
                } else if (cs.type == MD_INTER) {
                    full = md_inter_full_luma_cost(&P, &cuv, &cs, N, ycbf, frate, (const uint64_t *)dist, bits, &mc, &sc);
                } else {
                    full = md_intra_full_luma_cost_pslice(&P, N, ycbf, frate, dist[0], bits);
                }
            }
            /* the reference walks the candidates in order: an intra candidate after an inter one whose root cbf is 0 is not costed at all (full-loop escape, :4450-4460) and
             * keeps whatever its buffer held (here: the all-ones cost of the buffer's initialisation) */
            uint32_t prevRootCbf = 1;
            unsigned long long bestFullCost = 0xFFFFFFFFull, kept = 0;
            for (int g = 0; g < nfull; g++) {
                const int ty = __builtin_amdgcn_readlane(svtype, g);
                const uint32_t yc = md_rl(ycbf, g);
                const unsigned long long cs_ = md_readlane64(full, g);
                if (ty == MD_INTRA && prevRootCbf == 0)
                    continue;
                kept |= 1ull << g;
                if (Ph.full_loop_escape && ty == MD_INTER && cs_ < bestFullCost)
                    prevRootCbf = yc, bestFullCost = cs_;
            }
            MD_TR(35);
            MD_SUB(14);
            /* ProductFullModeDecision (:1995): the lowest full cost among the first full_count buffers of the order (the first of equal ones) */
            const unsigned long long fcost = (have && ((kept >> lane) & 1ull)) ? full : ~0ull;
            int wf = 0;
            {
                unsigned long long lowestCost = ~0ull;
                for (int f = 0; f < full_count && f < nfull; f++) { /* (buffers beyond the survivors keep the all-ones cost: never lower) */
                    const unsigned long long v = md_readlane64(fcost, f);
                    if (v < lowestCost)
                        wf = f, lowestCost = v;
                }
            }
            /* the winner's lane hands its sums to lane 0 */
            const unsigned long long w_cost = md_readlane64(fcost, wf), w_mc = md_readlane64(mc, wf), w_sc = md_readlane64(sc, wf), w_bits = md_readlane64(bits, wf),
                                     w_d0 = md_readlane64(dist[0], wf), w_d1 = md_readlane64(dist[1], wf), w_rate = md_readlane64(frate, wf);
            const uint32_t w_ycbf = md_rl(ycbf, wf), w_c0 = md_rl(sv.w[0], wf), w_c2 = md_rl(sv.w[2], wf), w_mv0 = md_rl(sv.w[4], wf), w_mv1 = md_rl(sv.w[5], wf);
            const bool w_kept = ((kept >> wf) & 1ull) != 0;
            const int wtype = (int)(w_c0 & 0xFF), wdir = (int)(w_c2 & 0xFF);
            int last_v = leaf, upd_v = 0; /* (lane 0's; the wave reads them by v_readlane - a hand-over through LDS is two dependent round trips on the chain) */
            if (lane == 0) {
                MdCu &u = M.S.cu[leaf];
                /* (a winner the escape left uncosted keeps the buffer's initial values: zeros, as ProductResetModeDecision leaves them) */
                M.S.local[leaf].cost = w_cost, M.S.local[leaf].full_distortion = w_kept ? (uint32_t)w_d0 : 0u;
                u.pred_mode = (uint8_t)wtype, u.skip_flag = 0, u.intra_luma_mode = (uint8_t)(wtype == MD_INTRA ? ((w_c0 >> 8) & 0xFF) : 0x1F);
                const uint32_t yc = w_kept ? w_ycbf : 0u;
                u.ycbf = (uint8_t)(N == 64 ? (yc & 0x1E) : (yc & 1));
                { /* inter_dir | merge_flag | merge_index | pad, mv[0], mv[1]: three words of the record, three stores */
                    static_assert(offsetof(MdCu, inter_dir) == 8 && offsetof(MdCu, merge_flag) == 9 && offsetof(MdCu, merge_index) == 10 && offsetof(MdCu, mv) == 12 && sizeof(MdMv) == 4,
                                  "the unit's record, words 2..4");
                    const bool wi = wtype == MD_INTER;
                    uint32_t *q = reinterpret_cast<uint32_t *>(&u.inter_dir);
                    q[0] = (wi ? (uint32_t)wdir : 3u) | ((wi ? (w_c2 >> 8) & 0xFFu : 0u) << 8) | (((w_c2 >> 16) & 0xFFu) << 16);
                    q[1] = wi && wdir != MD_L1 ? w_mv0 : 0u, q[2] = wi && wdir != MD_L0 ? w_mv1 : 0u;
                }
                u.merge_cost = w_kept ? w_mc : 0, u.skip_cost = w_kept ? w_sc : 0;
                u.y_coeff_bits = w_kept ? w_bits : 0, u.y_dist[0] = w_kept ? w_d0 : 0, u.y_dist[1] = w_kept ? w_d1 : 0;
                u.fast_luma_rate = w_rate, u.ycbf_mask = yc;
                M.S.local[leaf].mdc_index = (uint8_t)cuIdx;
                int cur = leaf, curIdx = cuIdx, last;
                /* CheckHighCostPartition (md_check_high_cost_partition, md_logic.h) with everything it may read requested AT ONCE (the parent's record, the earlier siblings'
                 * costs, the counters of the depth decision, the next-unit step): one LDS round trip where the rule's early exits make a chain of five */
                const int off = md_depth_offset(st.depth), parent = st.parent;
                const MdLocal pl = M.S.local[parent];
                const uint64_t sib1 = M.S.local[leaf >= off ? leaf - off : 0].cost, sib2 = M.S.local[leaf >= 2 * off ? leaf - 2 * off : 0].cost;
                const int split_now = u.split, g8 = M.S.g8, g16 = M.S.g16, step = M.next_step[cuIdx];
                int exitParent = -1;
                if (Lh.is_complete && st.depth != 0 && st.ordinal < 4 && !split_now && pl.tested) {
                    const MdStats ps = md_stats(parent);
                    const int ctx = (pl.left_mode > MD_INTRA ? 0 : pl.left_depth > ps.depth) + (pl.top_mode > MD_INTRA ? 0 : pl.top_depth > ps.depth);
                    const uint64_t srate = ps.depth < 3 ? (ctx == 0 ? sfb0 : ctx == 1 ? sfb1 : sfb2) : 0;
                    const uint64_t parentCost = pl.cost + (((uint64_t)Ph.full_lambda * srate + (1u << 22)) >> 23);
                    const uint64_t children = w_cost + (st.ordinal >= 2 ? sib1 : 0) + (st.ordinal >= 3 ? sib2 : 0);
                    if (children > parentCost)
                        exitParent = parent;
                }
                if (exitParent >= 0) {
                    cur = exitParent, curIdx = pl.mdc_index;
                    M.S.cu[exitParent].split = 0;
                    last = md_inter_depth_decision(&P, &M.S, exitParent, lcu_x, lcu_y, 1, 0);
                } else if (st.ordinal < 4 || st.depth == 0) {
                    /* ProductPerformInterDepthDecision (md_inter_depth_decision) of a unit that is not the last of its four siblings: no depth is compared, the unit becomes a
                     * leaf when the leaf list or StopSplitCondition says so and the counters of finished blocks move */
                    if (split_now == 0 || ((w_kept ? (uint32_t)w_d0 : 0u) < (st.depth == 0 ? ss_thr0 : st.depth == 1 ? ss_thr1 : st.depth == 2 ? ss_thr2 : 0u))) {
                        u.split = 0;
                        if (st.depth == 1)
                            M.S.g16 = (uint8_t)(g16 + 1);
                        else if (st.depth == 2)
                            M.S.g8 = (uint8_t)(g8 + 1);
                    }
                    last = leaf;
                } else { /* open loop: no reconstruction to wait for, the inter-depth decision follows at once */
                    last = md_inter_depth_decision(&P, &M.S, leaf, lcu_x, lcu_y, 0, ((w_kept ? (uint32_t)w_d0 : 0u) < (st.depth == 0 ? ss_thr0 : st.depth == 1 ? ss_thr1 : st.depth == 2 ? ss_thr2 : 0u)));
                }
                last_v = last, upd_v = M.S.cu[last].split == 0;
                /* the next unit (CalculateNextCuIndex :1261): the loop stands on `cur` - the tested unit, or the parent a partition exit fell back to */
                int nextIdx = curIdx;
                if (M.S.cu[cur].split || lh < 64)
                    nextIdx++;
                else
                    nextIdx += cur == leaf ? step : (int)M.next_step[curIdx];
                M.cu_idx = nextIdx;
                M.done = nextIdx >= Lh.leaf_count;
#ifdef MD_TRACE
                g_md_trace_on = D.trace && lcu == D.trace_lcu && nextIdx >= D.trace_unit && nextIdx < D.trace_unit + 2;
#endif
            }
            MD_TR(36);
            EP_WAVE_SYNC();
            MD_PROF(6);
            /* ModeDecisionUpdateNeighborArrays of the unit the decision ended on (at most 256 cells: this wave's lanes) */
            if (md_rl((uint32_t)upd_v, 0)) {
                const int last = (int)md_rl((uint32_t)last_v, 0);
                uint32_t w, m0, m1, md;
                MdStats ls = st;
                if (last == leaf) { /* the unit just decided (most updates): its record is in this wave's registers */
                    const bool wi = wtype == MD_INTER;
                    w = (uint32_t)wtype | ((wtype == MD_INTRA ? (w_c0 >> 8) & 0xFFu : 0x1Fu) << 8) | ((uint32_t)st.depth << 16);
                    m0 = wi && wdir != MD_L1 ? w_mv0 : 0u, m1 = wi && wdir != MD_L0 ? w_mv1 : 0u, md = wi ? (uint32_t)wdir : 3u;
                } else {
                    ls = md_stats(last);
                    const MdCu u = M.S.cu[last];
                    w = (uint32_t)u.pred_mode | ((uint32_t)u.intra_luma_mode << 8) | ((uint32_t)ls.depth << 16) | ((uint32_t)u.skip_flag << 24);
                    m0 = md_pack_mv(u.mv[0]), m1 = md_pack_mv(u.mv[1]), md = u.inter_dir;
                }
                const int cells = ls.size >> 2, lgc4 = ls.lg - 2;
                for (int e = lane; e < cells * cells; e += 64)
                    L.info[((ls.y >> 2) + (e >> lgc4) + 1) * 36 + (ls.x >> 2) + (e & (cells - 1)) + 1] = w;
                const int c8 = ls.size >> 3, lgc8 = ls.lg - 3;
                static_assert(sizeof(MdMvUnit) == 12, "three words: mv[0], mv[1], dir | avail << 8");
                for (int e = lane; e < c8 * c8; e += 64) {
                    uint32_t *q = reinterpret_cast<uint32_t *>(&M.V.mvu[((ls.y >> 3) + (e >> lgc8) + 1) * 18 + (ls.x >> 3) + (e & (c8 - 1)) + 1]);
                    q[0] = m0, q[1] = m1, q[2] = md;
                }
            }
            MD_TR(38);
        }
        __syncthreads();
        MD_TR(39);
        MD_PROF(8);
        cuIdx = M.cu_idx; /* (the next unit, or the end of the leaf list: one LDS round trip for both) */
        if (cuIdx >= (int)Lh.leaf_count)
            break;
    }
}
