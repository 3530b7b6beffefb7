/*
 * Device-resident mode decision + encode pass of whole pictures (include/svt_hevc_amd.h "Device-resident mode decision").
 *
 * Replaces, per LCU, what EncDecKernel's LCU loop runs between ModeDecisionConfigureLcu and the end of EncodePass
 * (Codec/EbEncDecProcess.c:2893-3023): ModeDecisionLcu (Codec/EbProductCodingLoop.c:4691-5114) followed by the LCU's EncodePass
 * (Codec/EbCodingLoop.c:2989; encdec_device.h) on the tree it decided, with the wavefront of AssignEncDecSegments
 * (Codec/EbEncDecProcess.c:1540) over the picture - ONE launch per picture.
 *
 * One 256-thread workgroup per LCU.  The LCU's mode-decision state lives in LDS: the mode decision's own luma reconstruction
 * (mdLumaReconNeighborArray as a picture plane: candidate reconstructions of the units decided so far) with a ring of neighbour samples,
 * the neighbour-array entries of the 4x4 cells (mode type | intra luma mode | depth | skip flag) with the same ring, the source block.
 * The LCU's own inputs (its records, the source block, the picture's controls and rate tables) are loaded BEFORE the workgroup waits for the LCU's neighbours;
 * what the neighbours left in the picture's maps follows the wait.  Per coding unit of the MdcLcuData_t leaf list (I pictures: waves 1..3 idle where P / B pictures
 * use them):
 *   lane 0        context generation, intra candidates                                       (md_logic.h - the text the CPU checker runs)
 *   P / B         beside it, from the unit's first moment: waves 1 and 2 fetch the spatial neighbours' motion (five lanes, a copy per wave) and lane 0 of each makes its
 *                 lists - wave 1 the AMVP candidates of both lists, wave 2 the merge candidates - while wave 3 builds the unit's intra reference (luma, and the chroma
 *                 pair of a CHROMA_MODE_FULL LCU, from SOURCE samples); then a lane per motion-estimation / merge candidate (md_choose_mvp, duplicate check),
 *                 survivors in the scalar order by ballot
 *   lane 0        MPM injection, buffer count;  wave 0: a lane per candidate - first fast loop (best distortion-ready candidate), evaluated flags,
 *                 the packed list of candidates that really need a prediction, prediction slots
 *   wave 0        (I pictures) intra reference of the unit: availability by ballot, substitution, [1 2 1] / strong smoothing   (8.4.4.2.2-3)
 *   4 waves       fast loop: ONE list of tasks (candidate, plane, tile) dealt to the waves - luma blocks (64x64 units: four 32x32 tiles), then, in CHROMA_MODE_FULL LCUs,
 *                 the Cb and Cr blocks of every evaluated candidate; inter prediction through md_predict_tile / ep_mc8_tile (encdec_device.h: LDS-staged reference windows,
 *                 v_dot4 / v_dot2 filters), intra prediction evaluated per sample in closed form (intra_device.h), SAD by v_sad_u8 on words, added to the candidate's
 *                 LDS accumulator
 *   wave 0        fast costs a lane per candidate (with the chroma distortion and the noise-class rule where the LCU has it), the candidate-buffer replay with the
 *                 buffers in lanes (v_readlane), PreModeDecision
 *   4 waves       full loop: a wave per surviving candidate (64x64 units: a wave per 32x32 transform unit) - residual row per lane, Estimate DCT in
 *                 registers, quantiser, coefficient-domain distortion, coefficient bits (a lane per 4x4 sub-block): the fused unit of the encode pass; CHROMA_MODE_FULL:
 *                 the survivors' chroma pairs (FullLoop_R + CuFullDistortionFastTuMode_R) as tasks on the least loaded waves
 *   wave 0        TuCalcCostLuma + full cost a lane per candidate (InterFullCost / MergeSkipFullCost / IntraFullCostPslice with the chroma terms where the LCU has
 *                 them); lane 0: ProductFullModeDecision, CheckHighCostPartition, (open loop) inter-depth decision
 *   wave 0        (closed loop) the winner's reconstruction (inverse transform + prediction);  lane 0: inter-depth decision
 *   all lanes     neighbour update
 * A 10-bit picture (k_md_picture<INTER, uint16_t>) is decided on the 8-MSB views of its source and reference pictures (MdPictureDev.src / .mref) and encoded
 * on the 10-bit samples (.src16, the picture object's 16-bit planes).
 * then the LCU's final tree becomes an SvtAmdLcuWork record and the encode pass of the LCU runs in the same workgroup.
 * Bounded by latency (an LCU's units are sequential, a picture's wavefront is <= (W/64+1)/2 LCUs wide), not by bytes: algorithmic HBM
 * traffic per LCU = 6 KB source + 6 KB OIS record in, 1.1 KB decisions + the encode pass's 24 KB out.
 */
/* This unit holds the kernels of the mode decision, the LCU's mode decision (md_lcu, with the unit loop of I pictures) and, at its end, the few host functions that launch
 * them; its other device functions are five headers - the LCU state (md_state.h), the intra leaves (md_intra.h), the transform leaves (md_txfm.h), the inter prediction
 * (md_inter.h), the unit loop of P / B pictures (md_units_inter.h) - beside the register lists (md_lists.h); the picture state, the launch budget and the entries are
 * md_picture.hip, which calls those functions (md_picture.h). */
#include "encdec_device.h"
#define MD_FN __host__ __device__ __forceinline__
#ifndef MD_RESTAGE_THR
#define MD_RESTAGE_THR 16 /* quarter samples: a neighbour's vector this far from the staged window's centre re-stages the window behind the wait (md_lcu) */
#endif
#include "md_logic.h"
#include "md_picture.h"
#include "md_lists.h"
#include "md_state.h"
#include "md_intra.h"
#include "md_txfm.h"
#include "md_inter.h"
#include "md_units_inter.h"

/* ModeDecisionLcu of one LCU: on return M.S holds the decisions, the picture's maps the LCU's final neighbour state */
/* what the LCU's mode decision reads that no other LCU of the picture writes (its records, its source): into LDS BEFORE the workgroup waits for the LCU's neighbours */
template <bool INTER>
__device__ __forceinline__ void md_lcu_inputs(const MdPictureDev &D, const SvtAmdMdPicture &P, int lcu, int lcu_x, int lcu_y, MdShared<INTER> &M)
{
    const int t = threadIdx.x;
    auto &L = M.L;
    const int lw = min(64, (int)P.width - lcu_x), lh = min(64, (int)P.height - lcu_y);
    for (int i = t; i < (int)sizeof(SvtAmdMdLcu); i += 256)
        ((uint8_t *)&M.lcu)[i] = ((const uint8_t *)&D.lcus[lcu])[i];
    static_assert(sizeof(SvtAmdCabacCost) % 4 == 0 && sizeof(SvtAmdMdPicture) % 4 == 0, "record sizes");
    for (int i = t; i < (int)(sizeof(SvtAmdMdPicture) / 4); i += 256)
        ((uint32_t *)&M.pic)[i] = ((const uint32_t *)D.P)[i];
    if (D.cost)
        for (int i = t; i < (int)(sizeof(SvtAmdCabacCost) / 4); i += 256)
            ((uint32_t *)&M.cost)[i] = ((const uint32_t *)D.cost)[i];
    static_assert(sizeof(RateTables) % 4 == 0, "record sizes");
    for (int i = t; i < (int)(sizeof(RateTables) / 4); i += 256)
        ((uint32_t *)&M.rt)[i] = ((const uint32_t *)&c_rt)[i];
    static_assert(sizeof(SvtAmdOisLcuResult) % 4 == 0 && sizeof(SvtAmdMeLcuResult) % 4 == 0 && sizeof(SvtAmdMeCuResult) % 4 == 0 && sizeof(SvtAmdTmvpLcu) % 8 == 0, "record sizes");
    for (int i = t; i < (int)(sizeof(SvtAmdOisLcuResult) / 4); i += 256)
        ((uint32_t *)&M.ois)[i] = ((const uint32_t *)&D.ois[lcu])[i];
    if constexpr (INTER) {
        for (int i = t; i < (int)(sizeof(M.V.me) / 4); i += 256)
            ((uint32_t *)M.V.me)[i] = ((const uint32_t *)D.me[lcu].pu)[i];
        static_assert(sizeof(EpRefPlanes) % 4 == 0, "record sizes");
        for (int i = t; i < (int)(2 * sizeof(EpRefPlanes) / 4); i += 256)
            ((uint32_t *)M.V.refs)[i] = ((const uint32_t *)D.mref)[i];
        static_assert(sizeof(SvtAmdMdInter) % 4 == 0, "record sizes");
        for (int i = t; i < (int)(sizeof(SvtAmdMdInter) / 4); i += 256)
            ((uint32_t *)&M.V.X)[i] = ((const uint32_t *)D.X)[i];
        if (D.X->tmvp_enable)
            for (int i = t; i < (int)(2 * sizeof(SvtAmdTmvpLcu) / 4); i += 256)
                ((uint32_t *)M.V.tmvp)[i] = ((const uint32_t *)&D.tmvp[lcu])[i];
    }
    for (int i = t; i < 64 * 64 / 4; i += 256) {
        const int y = i >> 4, x = (i & 15) * 4;
        uint32_t v = 0;
        if (x < lw && y < lh)
            v = *(const uint32_t *)(D.src[0] + (size_t)(lcu_y + y) * D.src_pitch[0] + lcu_x + x);
        *(uint32_t *)&L.src[y * 64 + x] = v;
    }
    if constexpr (INTER) { /* the chroma source: CHROMA_MODE_FULL candidates, and the merge / skip decisions behind the mode decision */
        for (int i = t; i < 2 * 32 * 32 / 4; i += 256) {
            const int p = i >> 8, e = i & 255, y = e >> 3, x = (e & 7) * 4;
            uint32_t v = 0;
            if (x < lw / 2 && y < lh / 2)
                v = *(const uint32_t *)(D.src[1 + p] + (size_t)(lcu_y / 2 + y) * D.src_pitch[1] + lcu_x / 2 + x);
            *(uint32_t *)&M.V.src_c[p][y * 32 + x] = v;
        }
    }
    __syncthreads();
    if (t == 0) {
        md_construct_cu_array(&M.S, &M.lcu);
        M.cu_idx = 0, M.done = 0;
    }
    if (t >= 64 && t < 64 + (int)M.lcu.leaf_count) /* (before the wait for the neighbours: off the chain) */
        M.next_step[t - 64] = (uint8_t)md_next_cu_step(&M.lcu, t - 64, md_stats(M.lcu.leaf_index[t - 64]).depth);
    if constexpr (INTER) {
        static_assert(sizeof(MdStats) == 8, "two words");
        if (t >= 128 && t < 128 + (int)M.lcu.leaf_count) {
            const int lf = M.lcu.leaf_index[t - 128];
            const MdStats s_ = md_stats(lf);
            uint32_t w_[2];
            __builtin_memcpy(w_, &s_, 8);
            M.V.unit_tab[t - 128] = make_uint4(w_[0], w_[1], (uint32_t)lf, 0u);
        }
    }
    if constexpr (INTER) {
        /* the spatial neighbours of every unit of the leaf list with the availability GenerateL0L1AmvpMergeLists derives from positions (EbAdaptiveMotionVectorPrediction.c:2256-2340:
         * scan order, array bounds, tile edges); whether the neighbour is an inter unit is the one thing left to the unit's own time */
        const bool tl = M.lcu.tile_left != 0, tt = M.lcu.tile_top != 0, tr = M.lcu.tile_right != 0;
        for (int i = t; i < 5 * (int)M.lcu.leaf_count; i += 256) {
            const int ci = i / 5, k = i - 5 * ci;
            const MdStats st = md_stats(M.lcu.leaf_index[ci]);
            const int N = st.size;
            const bool left = tl && st.x == 0, top = tt && st.y == 0, right = tr && ((st.x + N) & 63) == 0;
            const int px = k == 2 ? st.x + N : k == 3 ? st.x + N - 1 : st.x - 1, py = k == 0 ? st.y + N : k == 1 ? st.y + N - 1 : st.y - 1;
            bool ok = k == 0 ? md_bottom_left_ok(&st) && !left : k == 1 ? !left : k == 2 ? md_top_right_ok(&st) && !top && !right : k == 3 ? !top : !left && !top;
            const int cx = px >> 2, cy = py >> 2;
            if (cy >= 16 || cx >= 32 || (cy >= 0 && cx >= 16)) /* (MdLocal8T::info_at: never written before this LCU's units) */
                ok = false;
            const int ii = ok ? (cy + 1) * 36 + cx + 1 : 0, mi = ok ? ((py >> 3) + 1) * 18 + (px >> 3) + 1 : 0;
            M.V.nbtab[ci][k] = (uint32_t)ii | ((uint32_t)mi << 10) | ((uint32_t)ok << 18);
        }
    }
    if constexpr (INTER) { /* still before the wait for the LCU's neighbours: the reference samples its candidates will most likely read */
        const SvtAmdMeCuResult me0 = M.V.me[0];
        int16_t cmv[2][2];
        cmv[0][0] = me0.x_mv_l0, cmv[0][1] = me0.y_mv_l0, cmv[1][0] = me0.x_mv_l1, cmv[1][1] = me0.y_mv_l1;
        const bool use[2] = {true, P.slice_type == 0};
        ep_ref_windows_fill(D.mref, lcu_x, lcu_y, use, cmv, M.V.rw, t);
        const bool usec[2] = {M.lcu.chroma_encode_mode == 1, M.lcu.chroma_encode_mode == 1 && P.slice_type == 0};
        ep_ref_windows_fill_chroma(D.mref, lcu_x, lcu_y, usec, cmv, M.V.rwc, t);
    }
}

/* ModeDecisionLcu of one LCU (its inputs are in LDS: md_lcu_inputs): on return M.S holds the decisions, the picture's maps the LCU's final neighbour state */
template <bool INTER, bool PROF, bool IFREE = false>
__device__ __forceinline__ void md_lcu(const MdPictureDev &D, const SvtAmdMdPicture &Pg, int lcu, int lcu_x, int lcu_y, MdShared<INTER> &M)
{
    /* the picture's controls as the unit loop reads them: the copies md_lcu_inputs left beside the LCU in LDS, not the records in HBM (a unit's scalar stages read dozens
     * of these fields one after the other - each a round trip of its own from global memory) */
    const SvtAmdMdPicture &P = M.pic;
    (void)Pg;
    const bool prof_on = PROF && __builtin_amdgcn_readfirstlane((int)(D.prof != nullptr)) != 0;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    auto &L = M.L;
    const int W = (int)P.width, H = (int)P.height;
    const int lw = min(64, W - lcu_x), lh = min(64, H - lcu_y);
    const bool islice = P.slice_type == 2, open_loop = P.intra_md_open_loop != 0;
    /* ---- the LCU's surroundings (what its neighbours left in the picture's maps) into LDS ---- */
    for (int i = t; i < 17 * 36; i += 256) {
        const int cy = i / 36 - 1, cx = i - (cy + 1) * 36 - 1;
        uint32_t v = 0xFFFFFFFFu;
        if (cy < 0 || cx < 0) {
            const int px = lcu_x + 4 * cx, py = lcu_y + 4 * cy;
            v = (px < 0 || py < 0 || px >= W || py >= H) ? 0xFFFFFFFEu : D.md_info[(size_t)(py >> 2) * D.info_pitch + (px >> 2)];
        }
        L.info[i] = v;
    }
    if (!INTER) {
        for (int i = t; i < 130 + 64; i += 256) { /* ring samples: row -1 (x = -1 .. 128), column -1 */
            const int x = i < 130 ? i - 1 : -1, y = i < 130 ? -1 : i - 130;
            const int gx = lcu_x + x, gy = lcu_y + y;
            if (x < 128 && gx >= 0 && gy >= 0 && gx < W && gy < H)
                *L.at(x, y) = D.md_rec[(size_t)gy * D.md_pitch + gx];
        }
    }
    if constexpr (INTER) {
        for (int i = t; i < 9 * 18; i += 256) { /* the ring of motion-vector units: row -1 and column -1 */
            const int cy = i / 18 - 1, cx = i - (cy + 1) * 18 - 1;
            MdMvUnit u;
            u.mv[0].x = u.mv[0].y = u.mv[1].x = u.mv[1].y = 0, u.dir = 0, u.avail = 0, u.pad[0] = u.pad[1] = 0;
            const int px = lcu_x + 8 * cx, py = lcu_y + 8 * cy;
            if ((cy < 0 || cx < 0) && px >= 0 && py >= 0 && px < W && py < H) {
                const uint4 w = D.md_mv[(size_t)(py >> 3) * D.mv_pitch + (px >> 3)];
                u.mv[0].x = (int16_t)(w.x & 0xFFFF), u.mv[0].y = (int16_t)(w.x >> 16), u.mv[1].x = (int16_t)(w.y & 0xFFFF), u.mv[1].y = (int16_t)(w.y >> 16);
                u.dir = (uint8_t)w.z;
            }
            M.V.mvu[i] = u;
        }
    }
    __syncthreads();
    if constexpr (INTER) {
        /* The staged reference samples were centred on the 64x64 unit's motion-estimation vector before the wait.  The candidates the chain really predicts are mostly merge
         * candidates = the neighbours' vectors; where those lie elsewhere (periodic or low-texture content: the open-loop search and the decisions disagree) the window of
         * that list is staged again around the vector of the LCU's left / top neighbour - once per LCU instead of a round trip to HBM per candidate of every unit. */
        MdMvUnit nbu = M.V.mvu[1 * 18 + 0]; /* (x = -1, y = 0) */
        int have = (L.info_at(-1, 0) & 0xFF) == MD_INTER && !M.lcu.tile_left;
        if (!have) {
            nbu = M.V.mvu[0 * 18 + 1]; /* (x = 0, y = -1) */
            have = (L.info_at(0, -1) & 0xFF) == MD_INTER && !M.lcu.tile_top;
        }
        bool use[2] = {false, false};
        int16_t cmv[2][2] = {{0, 0}, {0, 0}};
        if (have) {
            const SvtAmdMeCuResult me0 = M.V.me[0];
            const int mex[2] = {me0.x_mv_l0, me0.x_mv_l1}, mey[2] = {me0.y_mv_l0, me0.y_mv_l1};
            for (int l = 0; l < (P.slice_type == 0 ? 2 : 1); l++)
                if ((nbu.dir == MD_BI || nbu.dir == l) && (abs(nbu.mv[l].x - mex[l]) > MD_RESTAGE_THR || abs(nbu.mv[l].y - mey[l]) > MD_RESTAGE_THR))
                    use[l] = true, cmv[l][0] = nbu.mv[l].x, cmv[l][1] = nbu.mv[l].y;
        }
        if (use[0] || use[1]) { /* (uniform: every thread read the same LDS words) */
            const int x0k[2] = {M.V.rw.x0[0], M.V.rw.x0[1]}, y0k[2] = {M.V.rw.y0[0], M.V.rw.y0[1]}, vk[2] = {M.V.rw.valid[0], M.V.rw.valid[1]};
            __syncthreads();
            ep_ref_windows_fill(D.mref, lcu_x, lcu_y, use, cmv, M.V.rw, t);
            if (t == 0)
                for (int l = 0; l < 2; l++)
                    if (!use[l]) /* the list that keeps its window (the fill marks an unused list invalid) */
                        M.V.rw.x0[l] = x0k[l], M.V.rw.y0[l] = y0k[l], M.V.rw.valid[l] = vk[l];
            __syncthreads();
        }
    }
    MD_PROF(0);
    const SvtAmdOisLcuResult *ois = &M.ois;
    const int pf = md_pf_mode(&P);
    /* ---- the LCU's units, one after the other: P / B pictures run md_units_inter, the loop below is the I pictures' alone ---- */
    if constexpr (INTER) {
        if (M.lcu.chroma_encode_mode == 1)
            md_units_inter<PROF, true, IFREE>(D, lcu, lcu_x, lcu_y, M);
        else
            md_units_inter<PROF, false, IFREE>(D, lcu, lcu_x, lcu_y, M);
    } else {
        for (;;) {
            MD_TR(10);
            /* ---- lane 0: the unit, its contexts and its candidates ---- */
            if (t == 0) {
                const int cuIdx = M.cu_idx, leaf = M.lcu.leaf_index[cuIdx];
                const MdStats st = md_stats(leaf);
                M.leaf = leaf;
                if (prof_on)
                    M.prof_depth = st.depth;
                M.S.local[leaf].tested = 1;
                M.S.cu[leaf].split = (uint8_t)((islice && st.depth == 0) ? 1 : M.lcu.leaf_split[cuIdx]);
                uint32_t l = L.info_at(st.x - 1, st.y), tp = L.info_at(st.x, st.y - 1);
                if ((M.lcu.tile_left && st.x == 0) || (l & 0xFF) == 0xFE)
                    l = 0xFFFFFFFFu;
                if ((M.lcu.tile_top && st.y == 0) || (tp & 0xFF) == 0xFE)
                    tp = 0xFFFFFFFFu;
                MdNeighbors Nb;
                Nb.left_mode = (uint8_t)l, Nb.left_intra = (uint8_t)(l >> 8), Nb.left_depth = (uint8_t)(l >> 16), Nb.left_skip = (uint8_t)(l >> 24);
                Nb.top_mode = (uint8_t)tp, Nb.top_intra = (uint8_t)(tp >> 8), Nb.top_depth = (uint8_t)(tp >> 16), Nb.top_skip = (uint8_t)(tp >> 24);
                md_context_generation(&M.S, leaf, st.y, &Nb);
                M.S.cu[leaf].split = (uint8_t)md_skip_small_cu(&P, &M.lcu, &M.S, leaf, st.depth);
                int ncand = 0;
                if (st.depth != 0 && (islice || st.depth == 3 || !M.lcu.restrict_intra_global_motion))
                    if (!(P.limit_intra && st.x == 0 && st.y == 0))
                        ncand = md_intra_candidates(&P, &M.lcu, ois, leaf, &st, M.cand);
                M.ncand = ncand; /* the intra candidates so far */
            }
            if (wave == 0)
                MD_TR(11);
            MD_SUB(0);
            MD_SUB(4);
            if (t == 0) {
                const int leaf = M.leaf;
                const MdStats st = md_stats(leaf);
                int ncand = M.ncand;
                uint32_t mpm[3] = {0, 0, 0};
                if (P.mpm_search && !M.lcu.restrict_intra_global_motion)
                    md_mpm_modes(M.S.cu[leaf].left_intra_mode, M.S.cu[leaf].top_intra_mode, mpm);
                int bufferTotal = md_nfl(&P, &M.lcu, st.size);
                ncand = md_mpm_injection(&P, &M.lcu, &st, M.cand, ncand, &bufferTotal, mpm);
                bufferTotal = ncand < bufferTotal ? ncand : bufferTotal;
                const int width = st.depth == 0 ? 5 : 8;
                M.ncand = ncand, M.buffer_total = bufferTotal, M.max_buffers = bufferTotal + 1 < width ? bufferTotal + 1 : width;
            }
            if (wave == 0)
                MD_TR(17);
            MD_SUB(5);
            if (wave == 0) { /* a lane per candidate (MD_MAX_CAND <= 64): what the candidate list implies for the loops below */
                EP_WAVE_SYNC();
                const int nc = M.ncand, lf = M.leaf;
                const MdStats s1 = md_stats(lf);
                const bool in = lane < nc;
                MdCand c = M.cand[in ? lane : 0];
                M.any_intra = __ballot(in && c.type == MD_INTRA) != 0;
                /* the first fast loop (EbProductCodingLoop.c:1948-1988): the best of the candidates whose distortion the open-loop stages left; the reference
                 * walks from the last candidate down with <=: the LOWEST index among equal costs */
                int bestFirst = -1;
                if (!P.single_fast_loop) {
                    const bool ready = in && c.dist_ready;
                    unsigned long long cost = ~0ull;
                    if (ready) {
                        uint64_t r;
                        cost = c.type == MD_INTER ? md_inter_fast_cost(&P, &s1, &M.S.cu[lf], &c, c.me_dist, &r)
                               : islice          ? md_intra_fast_cost_islice(&P, &s1, &M.S.cu[lf], c.intra_mode, c.me_dist, &r)
                                                 : md_intra_fast_cost_pslice(&P, &s1, &M.S.cu[lf], c.intra_mode, c.me_dist, &r);
                    }
                    /* few candidates are ready: a scalar walk over them instead of a 64-lane reduction */
                    unsigned long long m = ~0ull, rm = __ballot(ready);
                    while (rm) {
                        const int l = __ffsll((long long)rm) - 1;
                        rm &= rm - 1;
                        const unsigned long long v = md_readlane64(cost, l);
                        if (bestFirst < 0 || v < m)
                            m = v, bestFirst = l;
                    }
                }
                uint8_t e = (uint8_t)(in && (!c.dist_ready || lane == bestFirst || P.single_fast_loop));
                if (e && lane == bestFirst && c.type == MD_INTRA && open_loop)
                    e = 3; /* the open-loop distortion stands, no luma prediction (:1660, :2042) */
                if (in)
                    M.evaluated[lane] = e;
                {   /* what the fast loop really has to do: predict + measure the evaluated candidates that are neither most-probable-mode placeholders nor the open-loop
                     * intra candidate whose distortion stands (:2042).  The list is packed - a wave per LIST entry keeps all four waves on real work */
                    const bool heavy = in && e && !c.mpm && !(lane == bestFirst && c.type == MD_INTRA);
                    const unsigned long long hm = __ballot(heavy);
                    if (heavy)
                        M.heavy[__popcll(hm & ((1ull << lane) - 1ull))] = (uint8_t)lane;
                    if (in) /* the heavy candidates' distortion is summed up by the fast loop (several waves may add to it) */
                        M.sad[lane] = (!heavy && e && !c.mpm) ? c.me_dist : 0u;
                    if (lane == 0)
                        M.nheavy = __popcll(hm);
                }
                if (lane == 0)
                    M.best_first = bestFirst;
                MD_TR(18);
            }
            MD_SUB(6);
            __syncthreads();
            MD_TR(19);
            MD_PROF(1);
            const int leaf = M.leaf, ncand = M.ncand;
            const MdStats st = md_stats(leaf);
            const int N = st.size, lgN = st.lg, x0 = lcu_x + st.x, y0 = lcu_y + st.y;
            /* ---- wave 0: the unit's intra reference ---- */
            if (wave == 0 && M.any_intra) {
                if (open_loop)
                    md_build_refs_ol(D, M, st, x0, y0, W, H, lane);
                else
                    md_build_refs(M, st, lane);
            }
            __syncthreads();
            MD_PROF(2);
            if (prof_on && t == 0)
                M.prof[13] += (unsigned long long)ncand, M.prof[14] += 1, M.prof_d[M.prof_depth][13] += (unsigned long long)ncand, M.prof_d[M.prof_depth][14] += 1;
            /* ---- fast loop (ProductPerformFastLoop's second loop): the packed list of candidates dealt to the four waves, a wave per candidate ----
             * A task predicts its luma block (per sample in closed form), measures it against the source and adds its part to the candidate's distortion. */
            for (int k = wave, nheavy = M.nheavy; k < nheavy; k += 4) {
                const int c = M.heavy[k];
                MD_TR(20);
                const MdCand cd = M.cand[c];
                uint32_t sad = 0;
                if (cd.type != MD_INTER) {
                    const int mode = cd.intra_mode;
                    sad = md_intra_block(mode, N, lgN, (!open_loop && md_mode_filtered(mode, lgN)) ? M.reff : M.ref, 1, lane, &L.src[st.y * 64 + st.x], 64, nullptr);
                }
                sad = md_wave_sum(sad);
                MD_TR(23);
                MD_SUB(8);
                if (lane == 0 && sad)
                    atomicAdd(&M.sad[c], sad);
                MD_TR(24);
            }
            __syncthreads();
            MD_TR(25);
            MD_PROF(3);
            /* ---- wave 0: fast costs (a lane per candidate: MD_MAX_CAND <= 64), candidate buffers (a lane per buffer), PreModeDecision ---- */
            if (wave == 0) {
                const int i = lane;
                unsigned long long rate = 0, cst = ~0ull;
                int evl = 0;
                if (i < ncand) {
                    evl = M.evaluated[i];
                    if (evl) {
                        const uint64_t dist = M.cand[i].mpm ? 0 : M.sad[i];
                        const uint64_t distc = 0; /* luma-only candidates: no chroma distortion, no chroma weight */
                        const uint32_t cw = 0;
                        cst = M.cand[i].type == MD_INTER ? md_inter_fast_cost_c(&P, &st, &M.S.cu[leaf], &M.cand[i], dist, distc, cw, !M.lcu.cmplx_noise, (uint64_t *)&rate)
                              : islice                  ? md_intra_fast_cost_islice(&P, &st, &M.S.cu[leaf], M.cand[i].intra_mode, dist, (uint64_t *)&rate)
                                                        : md_intra_fast_cost_pslice_c(&P, &st, &M.S.cu[leaf], M.cand[i].intra_mode, dist, distc, cw, (uint64_t *)&rate);
                        if (M.cand[i].mpm)
                            cst = 0;
                    }
                    M.costs[i] = cst, M.fast_rate[i] = rate;
                }
                MD_TR(26);
                MD_SUB(9);
                /* md_fast_loop_buffers (md_logic.h; ProductPerformFastLoop's second loop, :1990-2179) with the buffers in lanes 0..7 instead of LDS: the candidates
                 * arrive from the last to the first, each goes into the buffer with the highest cost (an unused one first) = the FIRST buffer holding the maximum
                 * over [0, maxBuffers) - the reference's scan starts at buffer 0, moves on a strictly greater cost and stops at an unused (all-ones) one; its
                 * do-while looks at buffer 1 even when maxBuffers is 1.  Scalar, the replay of 35 intra candidates was a third of an I picture's time. */
                unsigned long long bcost = ~0ull;
                int bcand = -1, bpred = -1, evcount = 0, highest = 0;
                const int maxb = __builtin_amdgcn_readfirstlane(M.max_buffers < 2 ? 2 : M.max_buffers);
                for (int idx = __builtin_amdgcn_readfirstlane(ncand) - 1; idx >= 0; idx--) {
                    const unsigned long long c = md_readlane64(cst, idx);
                    const int ev = __builtin_amdgcn_readlane(evl, idx);
                    if (lane == highest) {
                        bcand = idx;
                        if (ev) {
                            bcost = c;
                            if (!(ev & 2))
                                bpred = idx;
                        }
                    }
                    evcount += ev != 0;
                    if (idx) { /* the first buffer holding the maximum: the buffers' costs read lane by lane (scalar) */
                        unsigned long long m = 0;
                        int h = 0;
    #pragma unroll
                        for (int b = 0; b < MD_MAX_BUF; b++)
                            if (b < maxb) {
                                const unsigned long long v = md_readlane64(bcost, b);
                                if (b == 0 || v > m)
                                    m = v, h = b;
                            }
                        highest = h;
                    }
                }
                MD_TR(27);
                MD_SUB(10);
                if (lane < MD_MAX_BUF) {
                    M.B.fast_cost[lane] = bcost, M.B.full_cost[lane] = ~0ull, M.B.cand[lane] = (int16_t)bcand, M.B.pred[lane] = (int16_t)bpred;
                    M.types[lane] = bcand >= 0 ? M.cand[bcand].type : 0, M.ycbf[lane] = 0, M.full_dist[lane] = 0, M.merge_cost[lane] = M.skip_cost[lane] = 0;
                    M.y_bits[lane] = M.y_dist[lane][0] = M.y_dist[lane][1] = 0;
                }
                if (lane == 0)
                    M.B.evaluated_count = evcount;
                EP_WAVE_SYNC();
                if (lane == 0) {
                    int bufferTotal = M.buffer_total;
                    bufferTotal = evcount < bufferTotal ? evcount : bufferTotal;
                    const int same = evcount == bufferTotal;
                    M.full_count = md_pre_mode_decision(&M.B, M.types, same ? bufferTotal : M.max_buffers, same, M.best);
                    M.nfull = M.full_count < bufferTotal ? M.full_count : bufferTotal;
                }
                MD_TR(28);
            }
            __syncthreads();
            MD_TR(29);
            MD_PROF(4);
            /* ---- full loop: a wave per surviving candidate (PerformFullLoop, :4351) ---- */
            const int nfull = M.nfull;
            for (int f = wave; f < nfull; f += 4) {
                MD_TR(30);
                const int b = M.best[f], ci = M.B.cand[b];
                const MdCand cd = M.cand[ci];
                /* the buffer's luma prediction: the candidate the fast loop predicted there, or - predictionIsReadyLuma == 0 - a fresh one */
                const bool fresh = ci == M.best_first && cd.type == MD_INTRA && open_loop && M.evaluated[ci];
                const int pci = (fresh || M.B.pred[b] < 0) ? ci : M.B.pred[b];
                const MdCand pc = M.cand[pci];
                uint8_t *pred = M.V.pred[b];
                int16_t *rc = M.V.recon_coeff[b];
                if (pc.type != MD_INTER) {
                    const int mode = pc.intra_mode;
                    md_intra_block(mode, N, lgN, (!open_loop && md_mode_filtered(mode, lgN)) ? M.reff : M.ref, 1, lane, nullptr, 0, pred);
                    EP_WAVE_SYNC();
                }
                MD_TR(31);
                MD_SUB(12);
                md_full_loop_cand(lane, N, &L.src[st.y * 64 + st.x], pred, N, rc, M.tiles[wave], M.qbuf[wave], P, M.cost, M.rt, cd.type, cd.intra_mode, pf, M.fl[b]);
                MD_TR(32);
                MD_SUB(13);
            }
            MD_TR(33);
            __syncthreads();
            MD_TR(34);
            MD_PROF(5);
            /* ---- wave 0: TuCalcCostLuma + the full cost of every surviving candidate (a lane each), then lane 0: ProductFullModeDecision, CheckHighCostPartition ---- */
            if (wave == 0) {
                const bool have = lane < nfull;
                int b = 0, ctype = 0;
                uint32_t ycbf = 0;
                unsigned long long bits = 0, dist[2] = {0, 0}, full = 0;
                uint64_t mc = 0, sc = 0;
                if (have) {
                    const SvtAmdMdPicture &PL = M.pic; /* the rate tables beside the LCU */
                    b = M.best[lane];
                    const int ci = M.B.cand[b];
                    const MdCand c = M.cand[ci];
                    ctype = c.type;
                    if (N == 64) {
                        for (int tu = 0; tu < 4; tu++)
                            md_tu_calc_cost(PL, M.fl[b][tu], c.type, 64, 32, tu + 1, &ycbf, &bits, dist);
                    } else {
                        md_tu_calc_cost(PL, M.fl[b][0], c.type, N, N, 0, &ycbf, &bits, dist);
                    }
                    if (M.lcu.chroma_encode_mode == 2 /* CHROMA_MODE_BEST */ || M.lcu.chroma_encode_mode == 1)
                        bits = md_pf_coeff_bits(pf, P.qp, bits);
                    if (c.type == MD_INTER)
                        full = md_inter_full_luma_cost(&PL, &M.S.cu[leaf], &c, N, ycbf, M.fast_rate[ci], (const uint64_t *)dist, bits, &mc, &sc);
                    else if (islice)
                        full = md_intra_full_luma_cost_islice(&PL, lgN, ycbf, M.fast_rate[ci], dist[0], bits);
                    else
                        full = md_intra_full_luma_cost_pslice(&PL, N, ycbf, M.fast_rate[ci], dist[0], bits);
                }
                /* the reference walks the candidates in order: an intra candidate after an inter one whose root cbf is 0 is not costed at all (full-loop escape, :4450-4460) and
                 * keeps whatever its buffer held */
                uint32_t prevRootCbf = 1;
                unsigned long long bestFullCost = 0xFFFFFFFFull, kept = 0;
                for (int g = 0; g < nfull; g++) {
                    const int ty = __shfl(ctype, g);
                    const uint32_t yc = __shfl(ycbf, g);
                    const unsigned long long cs = __shfl(full, g);
                    if (!islice && ty == MD_INTRA && prevRootCbf == 0)
                        continue;
                    kept |= 1ull << g;
                    if (P.full_loop_escape && !islice && ty == MD_INTER && cs < bestFullCost)
                        prevRootCbf = yc, bestFullCost = cs;
                }
                MD_TR(35);
                MD_SUB(14);
                if (have && ((kept >> lane) & 1ull)) {
                    M.ycbf[b] = ycbf, M.full_dist[b] = (uint32_t)dist[0], M.B.full_cost[b] = full;
                    M.merge_cost[b] = mc, M.skip_cost[b] = sc, M.y_bits[b] = bits, M.y_dist[b][0] = dist[0], M.y_dist[b][1] = dist[1];
                }
                EP_WAVE_SYNC();
            }
            if (t == 0) {
                int lowest = M.best[0];
                unsigned long long lowestCost = ~0ull;
                for (int f = 0; f < M.full_count; f++)
                    if (M.B.full_cost[M.best[f]] < lowestCost)
                        lowest = M.best[f], lowestCost = M.B.full_cost[M.best[f]];
                if (ncand > 0) {
                    const MdCand c = M.cand[M.B.cand[lowest]];
                    MdCu &u = M.S.cu[leaf];
                    M.S.local[leaf].cost = M.B.full_cost[lowest], M.S.local[leaf].full_distortion = M.full_dist[lowest];
                    u.pred_mode = c.type, u.skip_flag = 0, u.intra_luma_mode = (uint8_t)(c.type == MD_INTRA ? c.intra_mode : 0x1F);
                    u.ycbf = (uint8_t)(N == 64 ? (M.ycbf[lowest] & 0x1E) : (M.ycbf[lowest] & 1));
                    u.inter_dir = (uint8_t)(c.type == MD_INTER ? c.dir : 3), u.merge_flag = (uint8_t)(c.type == MD_INTER ? c.merge_flag : 0), u.merge_index = c.merge_index;
                    u.mv[0].x = u.mv[0].y = u.mv[1].x = u.mv[1].y = 0;
                    if (c.type == MD_INTER) {
                        if (c.dir != MD_L1)
                            u.mv[0] = c.mv[0];
                        if (c.dir != MD_L0)
                            u.mv[1] = c.mv[1];
                    }
                    u.merge_cost = M.merge_cost[lowest], u.skip_cost = M.skip_cost[lowest];
                    u.y_coeff_bits = M.y_bits[lowest], u.y_dist[0] = M.y_dist[lowest][0], u.y_dist[1] = M.y_dist[lowest][1];
                    u.fast_luma_rate = M.fast_rate[M.B.cand[lowest]], u.ycbf_mask = M.ycbf[lowest];
                }
                M.lowest = lowest;
                M.S.local[leaf].mdc_index = (uint8_t)M.cu_idx;
                const int exitParent = md_check_high_cost_partition(&P, &M.lcu, &M.S, leaf);
                M.do_recon = exitParent < 0 && ncand > 0 && !open_loop, M.exited = exitParent >= 0;
                if (exitParent >= 0) {
                    M.leaf = exitParent, M.cu_idx = M.S.local[exitParent].mdc_index;
                    M.S.cu[exitParent].split = 0;
                    M.last = md_inter_depth_decision(&P, &M.S, exitParent, lcu_x, lcu_y, 1, 0);
                } else if (open_loop) { /* no reconstruction to wait for: the inter-depth decision follows at once */
                    M.last = md_inter_depth_decision(&P, &M.S, leaf, lcu_x, lcu_y, 0, md_stop_split(&P, &M.lcu, st.depth, M.S.local[leaf].full_distortion));
                }
                if (exitParent >= 0 || open_loop)
                    M.update = M.S.cu[M.last].split == 0;
                MD_TR(36);
            }
            __syncthreads();
            MD_TR(37);
            MD_PROF(6);
            /* ---- wave 0: the winner's reconstruction ---- */
            if (M.do_recon && wave == 0) {
                const int b = M.lowest;
                uint8_t *dst = M.V.best_rec[st.depth] + st.y * 64 + st.x;
                if (M.S.cu[leaf].ycbf) {
                    switch (N) {
                    case 32: md_recon_unit<32>(lane, M.V.recon_coeff[b], M.V.pred[b], dst, M.tiles[0]); break;
                    case 16: md_recon_unit<16>(lane, M.V.recon_coeff[b], M.V.pred[b], dst, M.tiles[0]); break;
                    default: md_recon_unit<8>(lane, M.V.recon_coeff[b], M.V.pred[b], dst, M.tiles[0]); break;
                    }
                } else {
                    for (int e = lane; e < N * N; e += 64)
                        dst[(e >> lgN) * 64 + (e & (N - 1))] = M.V.pred[b][e];
                }
            }
            __syncthreads();
            /* ---- lane 0: inter-depth decision ---- */
            if (t == 0 && !open_loop) {
                if (!M.exited)
                    M.last = md_inter_depth_decision(&P, &M.S, leaf, lcu_x, lcu_y, 0, md_stop_split(&P, &M.lcu, st.depth, M.S.local[leaf].full_distortion));
                M.update = M.S.cu[M.last].split == 0;
            }
            __syncthreads();
            MD_PROF(7);
            /* ---- all lanes: ModeDecisionUpdateNeighborArrays of the unit the decision ended on ---- */
            if (M.update) {
                const int last = M.last;
                const MdStats ls = md_stats(last);
                const MdCu u = M.S.cu[last];
                const uint32_t w = (uint32_t)u.pred_mode | ((uint32_t)u.intra_luma_mode << 8) | ((uint32_t)ls.depth << 16) | ((uint32_t)u.skip_flag << 24);
                if (!open_loop) {
                    const uint8_t *srcp = M.V.best_rec[ls.depth];
                    for (int e = t; e < ls.size * ls.size; e += 256) {
                        const int y = e >> ls.lg, x = e & (ls.size - 1);
                        *L.at(ls.x + x, ls.y + y) = srcp[(ls.y + y) * 64 + ls.x + x];
                    }
                }
                const int cells = ls.size >> 2;
                for (int e = t; e < cells * cells; e += 256)
                    L.info[((ls.y >> 2) + e / cells + 1) * 36 + (ls.x >> 2) + e % cells + 1] = w;
            }
            MD_TR(38);
            __syncthreads();
            MD_TR(39);
            if (t == 0) {
                const int cur = M.leaf; /* the unit the loop stands on: the tested one, or the parent a partition exit fell back to */
                const MdStats cs = md_stats(cur);
                int cuIdx = M.cu_idx;
                if (M.S.cu[cur].split)
                    cuIdx++;
                else if (lh < 64)
                    cuIdx++;
                else
                    cuIdx += md_next_cu_step(&M.lcu, cuIdx, cs.depth);
                M.cu_idx = cuIdx;
                M.done = cuIdx >= M.lcu.leaf_count;
    #ifdef MD_TRACE
                g_md_trace_on = D.trace && lcu == D.trace_lcu && cuIdx >= D.trace_unit && cuIdx < D.trace_unit + 2;
                if (D.trace && lcu == D.trace_lcu)
                    D.trace[4 * (1 + MD_TRACE_N) + 3] += 0x10000ull + (g_md_trace_on ? 1 : 0) + ((unsigned long long)g_md_trace_n[0] << 32);
    #endif
            }
            __syncthreads();
            MD_PROF(8);
            if (M.done)
                break;
        }
    }
    /* ---- the LCU's state leaves LDS: neighbour maps of the picture + the decision record ---- */
    if (!INTER) {
        for (int i = t; i < 64 * 64 / 4; i += 256) {
            const int y = i >> 4, x = (i & 15) * 4;
            if (x < lw && y < lh)
                *(uint32_t *)(D.md_rec + (size_t)(lcu_y + y) * D.md_pitch + lcu_x + x) = *(const uint32_t *)L.at(x, y);
        }
    }
    for (int i = t; i < 16 * 16; i += 256) {
        const int cy = i >> 4, cx = i & 15;
        if (4 * cx < lw && 4 * cy < lh)
            D.md_info[(size_t)((lcu_y >> 2) + cy) * D.info_pitch + (lcu_x >> 2) + cx] = L.info[(cy + 1) * 36 + cx + 1];
    }
    if constexpr (INTER) {
        for (int i = t; i < 8 * 8; i += 256) {
            const int cy = i >> 3, cx = i & 7;
            if (8 * cx < lw && 8 * cy < lh) {
                const MdMvUnit u = M.V.mvu[(cy + 1) * 18 + cx + 1];
                uint4 w;
                w.x = (uint32_t)(uint16_t)u.mv[0].x | ((uint32_t)(uint16_t)u.mv[0].y << 16), w.y = (uint32_t)(uint16_t)u.mv[1].x | ((uint32_t)(uint16_t)u.mv[1].y << 16);
                w.z = u.dir, w.w = 0;
                D.md_mv[(size_t)((lcu_y >> 3) + cy) * D.mv_pitch + (lcu_x >> 3) + cx] = w;
            }
        }
    }
    if (D.out) {
        SvtAmdMdLcuOut &O = D.out[lcu];
        for (int i = t; i < SVT_AMD_MD_LEAVES; i += 256) {
            const MdCu u = M.S.cu[i];
            O.split[i] = u.split, O.tested[i] = M.S.local[i].tested, O.pred_mode[i] = u.pred_mode;
            O.intra_luma_mode[i] = u.intra_luma_mode, O.ycbf[i] = u.ycbf, O.cost[i] = M.S.local[i].cost;
            O.inter_dir[i] = u.inter_dir, O.merge_flag[i] = u.merge_flag, O.merge_index[i] = u.merge_index;
            O.mv[i][0][0] = u.mv[0].x, O.mv[i][0][1] = u.mv[0].y, O.mv[i][1][0] = u.mv[1].x, O.mv[i][1][1] = u.mv[1].y;
            O.merge_cost[i] = u.merge_cost, O.skip_cost[i] = u.skip_cost;
        }
    }
}

/* what EncodePass will do with the inter units of the LCU's final tree (Codec/EbCodingLoop.c:3838-3882): AMVP units as they are; merge units by the
 * merge / skip costs completed with chroma (AddChromaEncDec, Codec/EbProductCodingLoop.c:4158-4349: chroma prediction + chroma full loop +
 * MergeSkipFullCost), a wave per unit.  -> M.V.ep_kind[leaf] */
/* (IFREE: the chroma of the winning merge candidate is predicted at the rounded position, Codec/EbProductCodingLoop.c:4239) */
template <bool IFREE = false>
__device__ __forceinline__ void md_ep_kinds(const MdPictureDev &D, const SvtAmdMdPicture &Pg, MdShared<true> &M, int lcu_x, int lcu_y)
{
    const SvtAmdMdPicture &P = M.pic;
    (void)Pg;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t == 0) {
        int n = 0, it = 0;
        while (it < SVT_AMD_MD_LEAVES) {
            if (M.S.cu[it].split) {
                it++;
                continue;
            }
            const MdStats st = md_stats(it);
            if (lcu_x + st.x < (int)P.width && lcu_y + st.y < (int)P.height && M.S.cu[it].pred_mode == MD_INTER) {
                M.V.ep_kind[it] = M.S.cu[it].merge_flag ? SVT_AMD_EP_INTER_MERGE : SVT_AMD_EP_INTER_AMVP;
                if (M.S.cu[it].merge_flag && M.lcu.chroma_encode_mode == 1) /* CHROMA_MODE_FULL: the mode decision's merge / skip costs hold chroma already (EbCodingLoop.c:3840) */
                    M.V.ep_kind[it] = (uint8_t)md_ep_merge_kind(&M.V.X, &M.lcu, M.S.cu[it].merge_cost, M.S.cu[it].skip_cost);
                else if (M.S.cu[it].merge_flag && n < SVT_AMD_LCU_MAX_CUS)
                    M.V.fin_leaf[n++] = (uint8_t)it;
            }
            it += md_depth_offset(st.depth);
        }
        M.V.nfin = n;
    }
    __syncthreads(); /* (the LCU's chroma source is in LDS since md_lcu_inputs) */
    const int pf = md_pf_mode(&P);
    for (int i = wave; i < M.V.nfin; i += 4) {
        const int leaf = M.V.fin_leaf[i];
        const MdStats st = md_stats(leaf);
        const MdCu u = M.S.cu[leaf];
        const int N = st.size, Cn = N >> 1, T = N == 64 ? 16 : Cn, ntu = N == 64 ? 4 : 1;
        uint32_t cbf[2] = {0, 0};
        uint64_t bits[2] = {0, 0}, dist[2][2] = {{0, 0}, {0, 0}};
        MdCand cd; /* the unit's final prediction as a candidate: from the reference pictures as the mode decision reads them (their 8-MSB views of a 10-bit picture) */
        cd.type = MD_INTER, cd.dir = u.inter_dir, cd.mv[0] = u.mv[0], cd.mv[1] = u.mv[1];
        for (int p = 0; p < 2; p++) {
            uint8_t *pred = M.V.wpred[wave] + p * 1024;
            md_predict_inter_plane<IFREE>(M.V.refs, cd, lcu_x + st.x, lcu_y + st.y, N, 1 + p, lane, M.V.mc[wave], pred, 0, 1, &M.V.rw, &M.V.rwc);
            for (int tu = 0; tu < ntu; tu++) {
                const int ox = ntu == 1 ? 0 : (tu & 1) << 4, oy = ntu == 1 ? 0 : (tu >> 1) << 4;
                uint32_t nz;
                unsigned long long d[2], b;
                md_chroma_tu(lane, T, &M.V.src_c[p][((st.y >> 1) + oy) * 32 + (st.x >> 1) + ox], pred + oy * Cn + ox, Cn, M.tiles[wave], M.qbuf[wave], P, M.cost, M.rt, MD_INTER, 0,
                             1 + p, pf, &nz, d, &b);
                cbf[p] |= (uint32_t)(nz != 0) << (ntu == 1 ? 0 : tu + 1);
                bits[p] += b, dist[p][0] += d[0], dist[p][1] += d[1];
            }
        }
        if (lane == 0) {
            uint64_t mc, sc;
            md_merge_skip_full_cost(&P, &M.V.X, &u, N, cbf, bits, dist, &mc, &sc);
            M.V.ep_kind[leaf] = (uint8_t)md_ep_merge_kind(&M.V.X, &M.lcu, mc, sc);
        }
    }
    __syncthreads();
}

/* the EncDec input contract the decisions amount to (what svt_hook_encdec.c:fill_work builds on the host): the final tree in Z order */
template <bool INTER, typename T>
__device__ __forceinline__ void md_make_work(const MdPictureDev &D, const SvtAmdMdPicture &P, const MdShared<INTER> &M, int lcu_x, int lcu_y, typename EpTypes<T>::Work &Wk)
{
    const int t = threadIdx.x;
    const int lw = min(64, (int)P.width - lcu_x), lh = min(64, (int)P.height - lcu_y);
    if (t == 0) {
        Wk.lcu_x = (uint16_t)lcu_x, Wk.lcu_y = (uint16_t)lcu_y;
        Wk.slice_type = P.slice_type, Wk.temporal_layer = P.temporal_layer, Wk.constrained_intra = P.constrained_intra, Wk.strong_smoothing = P.strong_smoothing;
        Wk.tile_left = M.lcu.tile_left, Wk.tile_top = M.lcu.tile_top, Wk.tile_right = M.lcu.tile_right;
        Wk.full_lambda = P.full_lambda;
        Wk.luma_cbf_bits[0] = P.rates.lumaCbfBits[0], Wk.luma_cbf_bits[1] = P.rates.lumaCbfBits[1];
        Wk.luma_cbf_bits[2] = P.rates.lumaCbfBits[5], Wk.luma_cbf_bits[3] = P.rates.lumaCbfBits[6];
        Wk.pm_core = 0;
        int n = 0, it = 0;
        while (it < SVT_AMD_MD_LEAVES) {
            if (M.S.cu[it].split) {
                it++;
                continue;
            }
            const MdStats st = md_stats(it);
            if (lcu_x + st.x < (int)P.width && lcu_y + st.y < (int)P.height && n < SVT_AMD_LCU_MAX_CUS) {
                SvtAmdLcuCu &u = Wk.cu[n++];
                const MdCu &c = M.S.cu[it];
                u.x = st.x, u.y = st.y, u.size = st.size, u.pred_mode = c.pred_mode, u.intra_luma_mode = c.pred_mode == MD_INTRA ? c.intra_luma_mode : 0;
                u.bottom_left_ok = (uint8_t)md_bottom_left_ok(&st), u.top_right_ok = (uint8_t)md_top_right_ok(&st);
                u.qp = P.qp, u.chroma_qp = P.chroma_qp, u.leaf_index = (uint8_t)it, u.inter_dir = 0, u.inter_kind = 0, u.dz_offset = 0;
                u.mv[0][0] = u.mv[0][1] = u.mv[1][0] = u.mv[1][1] = 0;
                if (c.pred_mode == MD_INTER) {
                    u.inter_dir = c.inter_dir;
                    if constexpr (INTER)
                        u.inter_kind = M.V.ep_kind[it];
                    u.mv[0][0] = c.mv[0].x, u.mv[0][1] = c.mv[0].y, u.mv[1][0] = c.mv[1].x, u.mv[1][1] = c.mv[1].y;
                }
            }
            it += md_depth_offset(st.depth);
        }
        Wk.num_cus = (uint8_t)n;
    }
    if constexpr (sizeof(T) == 1) {
        for (int i = t; i < 64 * 64 / 4; i += 256)
            ((uint32_t *)Wk.src_y)[i] = ((const uint32_t *)M.L.src)[i];
        for (int i = t; i < 2 * 32 * 32; i += 256) {
            const int p = i >> 10, e = i & 1023, y = e >> 5, x = e & 31;
            uint8_t v = 0;
            if (x < lw / 2 && y < lh / 2)
                v = D.src[1 + p][(size_t)(lcu_y / 2 + y) * D.src_pitch[1] + lcu_x / 2 + x];
            (p ? Wk.src_cr : Wk.src_cb)[e] = v;
        }
    } else { /* the encode pass of a 10-bit picture codes the 10-bit source (EncodePassPackLcu's inputSample16bitBuffer, EbCodingLoop.c:2867); zero outside the picture */
        for (int i = t; i < 64 * 64; i += 256) {
            const int y = i >> 6, x = i & 63;
            Wk.src_y[i] = (x < lw && y < lh) ? D.src16[0][(size_t)(lcu_y + y) * D.src_pitch[0] + lcu_x + x] : (uint16_t)0;
        }
        for (int i = t; i < 2 * 32 * 32; i += 256) {
            const int p = i >> 10, e = i & 1023, y = e >> 5, x = e & 31;
            uint16_t v = 0;
            if (x < lw / 2 && y < lh / 2)
                v = D.src16[1 + p][(size_t)(lcu_y / 2 + y) * D.src_pitch[1] + lcu_x / 2 + x];
            (p ? Wk.src_cr : Wk.src_cb)[e] = v;
        }
    }
}

/* ONE launch per picture: persistent workgroups draw LCUs as tickets in wavefront order (k_encode_picture's scheme, encdec_kernels.hip).  md_done[lcu] = the LCU's
 * mode-decision state is in the picture's maps: what the mode decision of the right and the lower-left LCU waits for.  Behind it, off the chain, the workgroup completes
 * the merge / skip decisions with chroma and writes the LCU's work record; the ENCODE PASS of the picture is a kernel of its own (k_encode_picture, launched behind this
 * one on the same stream: round 6 - inlined here it cost this kernel 904 B of private segment per lane, 43 K of its 64 K instructions and a quarter of every workgroup's
 * time, for work that is off the picture's critical path and runs 2040 LCUs wide in ~1.5 ms when it is launched on its own).
 * The picture's descriptor (MdPictureDev) comes by POINTER and is copied to LDS once per workgroup: passed by value, its run-time-indexed arrays (src[1 + p], mref[l])
 * forced the whole record into the private segment (110 scratch stores in the prologue, a memory round trip at every use). */
template <bool INTER, typename T, bool PROF, bool IFREE = false>
__global__ __launch_bounds__(256) void k_md_picture(const MdPictureDev *__restrict__ Dp, typename EpTypes<T>::Work *__restrict__ works, int nlcu, int wl, unsigned *ticket,
                                                    unsigned *md_done, const unsigned *__restrict__ order, unsigned epoch)
{
    /* the LCU state as STATIC shared memory (its size is a compile-time constant): with `extern __shared__` every leaf function looked the dynamic segment's offset up
     * in a table in memory at its entry (llvm.amdgcn.dynlds.offset.table: a scalar load and its latency per call), and no access had an absolute address */
    __shared__ MdShared<INTER> M;
    __shared__ unsigned s_ticket;
    __shared__ MdPictureDev s_D;
    static_assert(sizeof(MdPictureDev) % 8 == 0, "copied as 8-byte words");
    for (int i = threadIdx.x; i < (int)(sizeof(MdPictureDev) / 8); i += 256)
        reinterpret_cast<unsigned long long *>(&s_D)[i] = reinterpret_cast<const unsigned long long *>(Dp)[i];
    __syncthreads();
    md_dct_operands_init(Dp->force_butterflies);
    const MdPictureDev &D = s_D;
    const SvtAmdMdPicture &P = *D.P;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0)
            s_ticket = atomicAdd(ticket, 1u);
        __syncthreads();
        if ((int)s_ticket >= nlcu)
            return;
        const int lcu = (int)order[s_ticket];
        const int lx = lcu % wl, ly = lcu / wl;
        const SvtAmdMdLcu &Lc = D.lcus[lcu];
        unsigned long long c_ticket = 0;
        md_lcu_inputs<INTER>(D, P, lcu, lx * 64, ly * 64, M);
        const int dep0 = Lc.tile_left ? -1 : lcu - 1;
        const int dep1 = Lc.tile_top ? -1 : (Lc.tile_right || lx + 1 >= wl) ? lcu - wl : lcu - wl + 1;
        if (threadIdx.x == 0) {
            c_ticket = (PROF && D.prof) ? __builtin_readcyclecounter() : 0;
            if (dep0 >= 0)
                while (__hip_atomic_load(&md_done[dep0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch)
                    __builtin_amdgcn_s_sleep(2);
            if (dep1 >= 0)
                while (__hip_atomic_load(&md_done[dep1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch)
                    __builtin_amdgcn_s_sleep(2);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
        unsigned long long c_wait = 0, c_md = 0;
        if (PROF && D.prof && threadIdx.x == 0) {
            c_wait = __builtin_readcyclecounter();
            for (int k = 0; k < 32; k++)
                M.prof[k] = 0;
            for (int k = 0; k < 128; k++)
                M.prof_d[0][k] = 0;
            M.prof_depth = 0;
            M.prof_t = M.prof_s = c_wait;
        }
#ifdef MD_TRACE
        if (threadIdx.x < 4)
            g_md_trace_n[threadIdx.x] = 0;
        if (threadIdx.x == 0)
            g_md_trace_on = D.trace && lcu == D.trace_lcu && D.trace_unit == 0;
        __syncthreads();
#endif
        md_lcu<INTER, PROF, IFREE>(D, P, lcu, lx * 64, ly * 64, M);
        __syncthreads();
#ifdef MD_TRACE
        if (D.trace && lcu == D.trace_lcu) {
            for (int i = threadIdx.x; i < 4 * (1 + MD_TRACE_N); i += 256) {
                const int w_ = i / (1 + MD_TRACE_N), k_ = i - w_ * (1 + MD_TRACE_N);
                D.trace[i] = k_ == 0 ? (unsigned long long)g_md_trace_n[w_] : g_md_trace[w_][k_ - 1];
            }
        }
        __syncthreads();
#endif
        if (threadIdx.x == 0) { /* the LCU's neighbour state is in the maps: the next LCUs' mode decisions may start */
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __hip_atomic_store(&md_done[lcu], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (PROF && D.prof && threadIdx.x == 0) {
            c_md = __builtin_readcyclecounter();
            unsigned long long *q = D.prof + 16 * (size_t)lcu;
            for (int k = 0; k < 9; k++)
                q[k] += M.prof[k];
            q[9] += c_md - M.prof_t;         /* the LCU's state leaving LDS */
            q[12] += c_wait - c_ticket;       /* waiting for the LCU's neighbours */
            q[13] += M.prof[13], q[14] += M.prof[14]; /* candidates of the fast loops / units tested */
            unsigned long long *q2 = D.prof + 16 * (size_t)D.prof_lcus + 16 * (size_t)lcu; /* the sub-stage sums follow the stage sums of all LCUs */
            for (int k = 0; k < 16; k++)
                q2[k] += M.prof[16 + k];
            unsigned long long *q3 = D.prof + 32 * (size_t)D.prof_lcus + 128 * (size_t)lcu; /* ... and both by depth */
            for (int k = 0; k < 128; k++)
                q3[k] += M.prof_d[0][k];
            q[15] += 1;
        }
        if (D.encode) {
            if constexpr (INTER)
                md_ep_kinds<IFREE>(D, P, M, lx * 64, ly * 64);
            md_make_work<INTER, T>(D, P, M, lx * 64, ly * 64, works[lcu]);
            if (PROF && D.prof && threadIdx.x == 0)
                D.prof[16 * (size_t)lcu + 10] += __builtin_readcyclecounter() - c_md; /* merge / skip decisions with chroma + the work record */
        }
    }
}

/* every static __shared__ object k_md_picture holds beside the LCU state: the picture's descriptor (s_D), the ticket (s_ticket), the forward transforms' operands and
 * their debug switch (md_dct_operands_init), in -DMD_TRACE builds the trace buffers (encdec_device.h); 64 bytes for the objects' alignment */
#ifdef MD_TRACE
constexpr size_t MD_LDS_TRACE = sizeof(g_md_trace) + sizeof(g_md_trace_n) + sizeof(g_md_trace_on);
#else
constexpr size_t MD_LDS_TRACE = 0;
#endif
constexpr size_t MD_LDS_BESIDE = sizeof(MdPictureDev) + sizeof(unsigned) + sizeof(s_dct_op) + sizeof(s_md_force_bfly) + MD_LDS_TRACE + 64;
static_assert(sizeof(MdShared<true>) + MD_LDS_BESIDE <= 160 * 1024 && sizeof(MdShared<false>) + MD_LDS_BESIDE <= 160 * 1024,
              "the LCU state and the kernel's other shared objects have to fit the 160 KB of LDS of a CU");

/* the 8 most significant bits of 10-bit samples in 16-bit words (UnPack8BitDataSafeSub, C_DEFAULT/EbPackUnPack_C.c:203: sample >> 2): eight samples a thread */
__global__ __launch_bounds__(256) void k_msb_view(const uint16_t *__restrict__ in, uint8_t *__restrict__ out, size_t n)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i + 8 <= n) {
        const uint4 v = *(const uint4 *)(in + i);
        uint2 o;
        o.x = ((v.x >> 2) & 0xffu) | ((v.x >> 10) & 0xff00u) | (((v.y >> 2) & 0xffu) << 16) | (((v.y >> 18) & 0xffu) << 24);
        o.y = ((v.z >> 2) & 0xffu) | ((v.z >> 10) & 0xff00u) | (((v.w >> 2) & 0xffu) << 16) | (((v.w >> 18) & 0xffu) << 24);
        *(uint2 *)(out + i) = o;
    } else {
        for (size_t k = i; k < n; k++)
            out[k] = (uint8_t)(in[k] >> 2);
    }
}
/* a source plane from page-locked HOST memory into HBM by a kernel of the call's own stream (the device reads the host over PCIe): the runtime's
 * hipMemcpyAsync of such a plane - a DMA-engine transfer - blocked the calling thread for one to four mode-decision kernel durations whenever other
 * pictures' kernels were running (profiles/r05_y: 50 - 420 ms inside the call, a tenth of the calls); a launch never does.  src: any alignment; dst: 16 bytes */
typedef uint4 __attribute__((aligned(1))) md_u128u;
__global__ __launch_bounds__(256) void k_md_fetch_plane(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, size_t bytes)
{
    const size_t n16 = bytes >> 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256)
        *(uint4 *)(dst + i * 16) = *(const md_u128u *)(src + i * 16);
    if (blockIdx.x == 0 && threadIdx.x < (bytes & 15))
        dst[(n16 << 4) + threadIdx.x] = src[(n16 << 4) + threadIdx.x];
}

/* test (svt_amd_debug_md_lists_batch): the unit loop's motion-vector lists on single units, a lane per job.  The lists, the temporal candidate, the scale factors and the
 * predictor choice are md_units_inter's own __device__ functions (md_list_consts, md_tmvp_position, md_amvp_one_list, md_temporal_mvp_dev, md_merge_list_regs,
 * md_choose_mvp_one) on the neighbours packed as wave 1 / wave 2 pack them; what is written here is only what carries a job to them and their results out.  The two
 * motion-field records of a job (this LCU, the LCU to its right) are gathered into a private pair: the functions index them as one array. */
static_assert(sizeof(SvtAmdMdListNb) == sizeof(MdMvUnit) && offsetof(SvtAmdMdListNb, dir) == offsetof(MdMvUnit, dir) && offsetof(SvtAmdMdListNb, avail) == offsetof(MdMvUnit, avail),
              "a job's neighbour is an MdMvUnit");
#define MD_NB_VALS(w0, w1, w2) w0[MD_A0], w1[MD_A0], w2[MD_A0], w0[MD_A1], w1[MD_A1], w2[MD_A1], w0[MD_B0], w1[MD_B0], w2[MD_B0], w0[MD_B1], w1[MD_B1], w2[MD_B1], w0[MD_B2], w1[MD_B2], w2[MD_B2]
__global__ __launch_bounds__(64) void k_md_lists_batch(const SvtAmdMdListJob *__restrict__ jobs, const SvtAmdTmvpLcu *__restrict__ pool, SvtAmdMdListOut *__restrict__ outs, uint32_t n)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n)
        return;
    const SvtAmdMdListJob J = jobs[i];
    SvtAmdMdPicture P; /* (the functions read width, height and slice_type of it) */
    P.width = J.width, P.height = J.height, P.slice_type = J.slice_type;
    SvtAmdMdInter X;
    __builtin_memset(&X, 0, sizeof(X));
    X.picture_number = J.picture_number, X.ref_poc[0] = J.ref_poc[0], X.ref_poc[1] = J.ref_poc[1], X.colocated_poc = J.colocated_poc;
    X.colocated_pu_ref_list = J.colocated_pu_ref_list, X.is_low_delay = J.is_low_delay, X.tmvp_enable = J.has_field;
    SvtAmdTmvpLcu field[2];
    field[0] = pool[J.pool[0]], field[1] = pool[J.pool[1]];
    const SvtAmdTmvpLcu *map = J.has_field ? field : nullptr;
    const int x0 = J.ox, y0 = J.oy, N = J.size, totalMerge = J.total_merge;
    const MdListConsts K = md_list_consts(P, X);
    MdTmvpPos tp;
    tp.bottom_right = 0, tp.lcu_offset = 0, tp.unit = 0, tp.pad = 0;
    if (map)
        tp = md_tmvp_position(&P, map, x0, y0, N);
    uint32_t w0[5], w1[5], w2[5]; /* mv[0], mv[1], dir | avail << 8: zero when the neighbour is not available */
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const SvtAmdMdListNb &u = J.nb[k];
        MdMv m0, m1;
        m0.x = u.mv[0][0], m0.y = u.mv[0][1], m1.x = u.mv[1][0], m1.y = u.mv[1][1];
        w0[k] = u.avail ? md_pack_mv(m0) : 0u, w1[k] = u.avail ? md_pack_mv(m1) : 0u, w2[k] = u.avail ? (uint32_t)u.dir | 0x100u : 0u;
    }
    SvtAmdMdListOut o;
    __builtin_memset(&o, 0, sizeof(o));
    MdMv tv[2];
    bool tok[2] = {false, false};
    MdMv cmv[2];
#pragma unroll
    for (int l = 0; l < 2; l++) {
        uint32_t pa0, pa1;
        const int num = md_amvp_one_list(K, X, MD_NB_VALS(w0, w1, w2), map, tp, l, &pa0, &pa1);
        MdMv al[3];
        al[0] = md_unpack_mv(pa0), al[1] = md_unpack_mv(pa1), al[2] = al[1];
        o.amvp[l][0][0] = al[0].x, o.amvp[l][0][1] = al[0].y, o.amvp[l][1][0] = al[1].x, o.amvp[l][1][1] = al[1].y;
        o.amvp_count[l] = (uint8_t)num;
        cmv[l].x = J.me_mv[l][0], cmv[l].y = J.me_mv[l][1];
        if (J.me_dir == MD_BI || J.me_dir == l) {
            MdMv mvp;
            mvp.x = mvp.y = 0;
            md_choose_mvp_one(P, (uint32_t)x0, (uint32_t)y0, al, num, &cmv[l], &o.mvp_idx[l], &mvp);
            o.cand_mv[l][0] = cmv[l].x, o.cand_mv[l][1] = cmv[l].y, o.mvp[l][0] = mvp.x, o.mvp[l][1] = mvp.y;
        }
        tv[l].x = tv[l].y = 0;
        if (map && (l == 0 || K.bslice)) {
            tok[l] = md_temporal_mvp_dev(X, map, tp, l, &tv[l]);
            if (!tok[l])
                tv[l].x = tv[l].y = 0;
        }
    }
    MdMerge5 mg;
    md_merge_list_regs(K, MD_NB_VALS(w0, w1, w2), map != nullptr, tok[0], md_pack_mv(tv[0]), md_pack_mv(tv[1]), totalMerge, mg);
    o.merge_count = (uint8_t)totalMerge; /* (the list is always filled up to the count wanted) */
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const MdMv v0 = md_unpack_mv(mg.g0[k]), v1 = md_unpack_mv(mg.g1[k]);
        o.merge_dir[k] = (uint8_t)mg.gd[k];
        o.merge_mv[k][0][0] = v0.x, o.merge_mv[k][0][1] = v0.y, o.merge_mv[k][1][0] = v1.x, o.merge_mv[k][1][1] = v1.y;
    }
    outs[i] = o;
}
#undef MD_NB_VALS

/* ---- what md_picture.hip calls (md_picture.h) ---------------------------------------------------------------------------- */
int svt_amd_md_kernel_rate_tables(int device) { return rate_tables_once(device); }

int svt_amd_md_kernel_msb_view(hipStream_t st, const void *in16, uint8_t *out8, size_t samples)
{
    if (!samples)
        return SVT_AMD_OK;
    hipLaunchKernelGGL(k_msb_view, dim3((unsigned)((samples + 2047) / 2048)), dim3(256), 0, st, (const uint16_t *)in16, out8, samples);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

int svt_amd_md_kernel_fetch_plane(hipStream_t st, int workgroups, uint8_t *d_dst, const uint8_t *src, size_t bytes)
{
    hipLaunchKernelGGL(k_md_fetch_plane, dim3((unsigned)workgroups), dim3(256), 0, st, d_dst, src, bytes);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

int svt_amd_md_kernel_lists_batch(hipStream_t st, const SvtAmdMdListJob *d_jobs, const SvtAmdTmvpLcu *d_pool, SvtAmdMdListOut *d_outs, uint32_t n)
{
    hipLaunchKernelGGL(k_md_lists_batch, dim3((n + 63u) / 64u), dim3(64), 0, st, d_jobs, d_pool, d_outs, n);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

int svt_amd_md_kernel_lds_bytes(int inter) { return (int)(inter ? sizeof(MdShared<true>) : sizeof(MdShared<false>)) + (int)sizeof(MdPictureDev); }

int svt_amd_md_kernel_trace_words(void)
{
#ifdef MD_TRACE
    return 4 * (1 + MD_TRACE_N) + 4;
#else
    return 0;
#endif
}

template <bool INTER, typename T, bool PROF, bool IFREE>
static int md_launch_instance(const MdPictureLaunch &l)
{
    hipLaunchKernelGGL((k_md_picture<INTER, T, PROF, IFREE>), dim3((unsigned)l.grid), dim3(256), 0, l.st, l.d_D, (typename EpTypes<T>::Work *)l.d_works, l.n_active, l.wl,
                       l.ticket, l.md_done, l.order, l.epoch);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

/* the instance of k_md_picture for the picture: I or P / B, 8 or 16 bits a sample; the P / B kernels exist with and without the stage marks, the 8-bit ones also
 * interpolation-free (a picture coded without sub-sample search; 8-bit pictures only, the entries see to it) */
int svt_amd_md_kernel_launch(const MdPictureLaunch &l)
{
    if (l.inter && l.bps == 1 && l.ifree)
        return !l.profiled ? md_launch_instance<true, uint8_t, false, true>(l) : md_launch_instance<true, uint8_t, true, true>(l);
    if (l.inter && l.bps == 1)
        return !l.profiled ? md_launch_instance<true, uint8_t, false, false>(l) : md_launch_instance<true, uint8_t, true, false>(l);
#ifdef MD_INTER8_ONLY
    return SVT_AMD_ERR_BAD_PARAM;
#else
    if (l.bps == 1)
        return md_launch_instance<false, uint8_t, true, false>(l);
    if (l.inter)
        return !l.profiled ? md_launch_instance<true, uint16_t, false, false>(l) : md_launch_instance<true, uint16_t, true, false>(l);
    return md_launch_instance<false, uint16_t, true, false>(l);
#endif
}
