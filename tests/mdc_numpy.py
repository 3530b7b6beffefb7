"""Plain-Python restatement of the mode-decision configuration (the records of tests/mdc_records.py), written from the text
of the reference: ModeDecisionConfigurationKernel (Codec/EbModeDecisionConfigurationProcess.c:1905) and what it calls there and in
Codec/EbModeDecisionConfiguration.c (EarlyModeDecisionLcu :1059).  Loops run in the reference's order and every EB_U32 expression is kept to 32 bits, so the
wrapped differences and products of DeriveLcuScore, PerformOutlierRemoval and SetLcuBudget come out as the reference computes them.  Pinned on the
reference's own results by tests/test_mdc_cpu.py."""
import numpy as np

import mdc_records as R
from mdc_records import MD_SCAN, MD_TO_RASTER

U32 = 0xFFFFFFFF
# [hierarchicalLevels][temporalLayerIndex]; entries the reference's initialisers leave out are 0
GLOBAL_MOTION_THRESHOLD = ((2, 0, 0, 0, 0, 0), (4, 2, 0, 0, 0, 0), (8, 4, 2, 0, 0, 0), (16, 8, 4, 2, 0, 0), (32, 16, 8, 4, 2, 0), (64, 32, 16, 8, 4, 2))
ADP_LUMINOSITY_CHANGE_TH = ((2, 0, 0, 0, 0, 0), (2, 2, 0, 0, 0, 0), (3, 2, 2, 0, 0, 0), (3, 3, 2, 2, 0, 0), (4, 3, 3, 2, 2, 0), (4, 4, 3, 3, 2, 2))
INTRA_AREA_TH_CLASS_1 = ((20, 0, 0, 0, 0, 0), (30, 20, 0, 0, 0, 0), (40, 30, 20, 0, 0, 0), (50, 40, 30, 20, 0, 0), (50, 40, 30, 20, 10, 0), (50, 40, 30, 20, 10, 10))
MOD_QP_OFFSET_LAYER_ARRAY = ((1, 0, 0, 0, 0, 0), (5, 6, 0, 0, 0, 0), (3, 4, 5, 0, 0, 0), (1, 3, 5, 5, 0, 0), (1, 3, 5, 5, 6, 0), (1, 3, 5, 5, 6, 7))
# costDepthMode by LCU depth mode (ConfigureAdp :1288)
COST = {R.LCU_FULL85: 155, R.LCU_FULL84: 155, R.LCU_BDP: 129, R.LCU_LIGHT_BDP: 123, R.LCU_OPEN_LOOP: 110, R.LCU_LIGHT_OPEN_LOOP: 106, R.LCU_AVC: 138,
        R.LCU_LIGHT_AVC: 122, R.LCU_PRED_OPEN_LOOP: 100, R.LCU_PRED_OPEN_LOOP_1_NFL: 97}
P_, Pp1, Pp2, Pp3, Pm1, Pm2, Pm3 = 1, 2, 4, 8, 16, 32, 64
NDP_NREF = ((P_ + Pp1 + Pp2, P_ + Pp1, P_ + Pp1, P_ + Pm1),) * 3 + ((P_ + Pp1, P_ + Pp1, P_ + Pp1, P_ + Pm1),) * 3
NDP_FAST = ((P_ + Pp1 + Pp2, P_ + Pp1, P_ + Pp1, P_ + Pm1),) + ((P_, P_ + Pp1, P_ + Pp1, P_ + Pm1),) * 2 + ((P_, P_, P_, P_ + Pm1),) * 3
DEPTH_OFFSET = (85, 21, 5, 1)
RASTER_TO_MD = [int(np.flatnonzero(MD_TO_RASTER == k)[0]) for k in range(85)]
PARENT_CU_INDEX = (0, 0, 0, 0, 1, 2, 3, 5, 0, 1, 2, 3, 10, 0, 1, 2, 3, 15, 0, 1, 2, 3) + (21, 0, 0, 1, 2, 3, 5, 0, 1, 2, 3, 10, 0, 1, 2, 3, 15, 0, 1, 2, 3) + \
    (42, 0, 0, 1, 2, 3, 5, 0, 1, 2, 3, 10, 0, 1, 2, 3, 15, 0, 1, 2, 3) + (36, 0, 0, 1, 2, 3, 5, 0, 1, 2, 3, 10, 0, 1, 2, 3, 15, 0, 1, 2, 3)
# EbHevcIncrementalCount by raster index: 4 at the last unit of every group of four
INCREMENTAL_COUNT = [0] + [4] * 4 + [4 if (k & 1) and (k >> 2 & 1) else 0 for k in range(16)] + [4 if (k & 3) == 3 and (k >> 3 & 3) == 3 else 0 for k in range(64)]


def _s8(v):
    v &= 0xFF
    return v - 256 if v & 0x80 else v


def _s32(v):
    v &= U32
    return v - (1 << 32) if v & 0x80000000 else v


def mv_bits(x, y):
    """mvBitTable[x][y] (Codec/EbLambdaRateTables.h) as csrc/md_logic.h md_mv_bits has it"""
    core = ((73744, 128728, 203592), (130975, 178780, 253644), (202683, 253623, 321933))[min(x, 2)][min(y, 2)]
    lx, ly = (x.bit_length() - 2 if x >= 4 else 0), (y.bit_length() - 2 if y >= 4 else 0)
    return core + 65536 * (lx + ly)


def inter_cu_rate(direction, mv):
    """MdcInterCuRate (Codec/EbModeDecisionConfiguration.c:307)"""
    c = [min(abs(int(v)), 499) for v in mv]
    if direction == 1:
        return 86440 + 23196 + mv_bits(c[2], c[3])
    if direction == 2:
        return 86440 + 46392 + mv_bits(c[0], c[1]) + mv_bits(c[2], c[3])
    return 86440 + 23196 + mv_bits(c[0], c[1])


def picture_signals(rec, jb):
    """:1949-1975, SetSliceAndPictureChromaQpOffsets (:112), AdaptiveDlfParameterComputation (:175) -> the first eight fields of the picture record"""
    sp, noise = rec["sbo_pic"][0], int(rec["noise_pic"][0]["pic_noise_class"])
    grass, th = int(sp["grass_percentage"]), (1 if jb["ndth"] == 0 else 3)
    pan, tilt, homog = jb["pan"], jb["tilt"], jb["homog"]
    scene = 0
    if not pan and not tilt and 0 < grass <= 35 and noise >= th and homog < 50:
        scene = 1
    if pan and not tilt and 35 < grass <= 70 and noise >= th and homog < 50:
        scene = 2
    adjust = int(not pan and not tilt and 2 < grass <= 35 and homog < 70 and int(sp["zz_cost_average"]) > 15 and noise >= th)
    if noise >= 7:
        offset = 10
    elif noise >= 5:
        offset = 8
    else:
        offset = max(-12, min(12, MOD_QP_OFFSET_LAYER_ARRAY[jb["hier"]][jb["layer"]] - 3))
    high_intra = 0
    if jb["slice_type"] == R.B:
        if jb["layer"] == 0:
            high_intra = int(int(sp["intra_coded_block_probability"]) > INTRA_AREA_TH_CLASS_1[jb["hier"]][0])
        else:
            high_intra = int(bool(jb["ref_skip0"] or jb["ref_skip1"]))
    return scene, adjust, high_intra, offset


def aura_detection(w, h, rec, jb):
    """AuraDetection / AuraDetection64x64 (:791-939)"""
    wl, hl, col, row, complete, edge = R.geometry(w, h)
    n = wl * hl
    aura = np.full(n, R.INVALID_AURA_STATUS, np.uint8)
    if jb["slice_type"] != R.B:
        return aura
    pu = rec["me"]["pu"]
    th0 = 15 if jb["ref"] or jb["cls"] == 3 else 14
    th1 = 23
    if jb["qp"] > 38:
        th0, th1 = th0 << 2, th1 << 2
    gmt = GLOBAL_MOTION_THRESHOLD[jb["hier"]][jb["layer"]]
    for i in range(n):
        if not (col[i] > 0 and col[i] < wl - 1 and row[i] < hl - 1):
            continue
        status = 0
        if not edge[i]:
            mv0, mv1 = (0, 0), (0, 0)
            u = pu[i][0]
            for k in range(int(u["total"])):
                if u["direction"][k] == 0:
                    mv0 = (int(u["mv"][0]), int(u["mv"][1]))
                if u["direction"][k] == 1:
                    mv1 = (int(u["mv"][2]), int(u["mv"][3]))
            cur = int(u["distortion"][0])
            if cur > 64 * 64 and (abs(mv0[0]) > gmt or abs(mv0[1]) > gmt or abs(mv1[0]) > gmt or abs(mv1[1]) > gmt):
                d = lambda off: int(pu[i + off][0]["distortion"][0])  # noqa: E731
                top, top_l, top_r, left = d(-wl), d(-wl - 1), d(-wl + 1), d(-1)
                top_r = top_r if col[i] < wl - 2 else cur
                right = top_r if col[i] < wl - 2 else cur            # :888: assigned from topRDist; the right neighbour's distortion is never used
                local = min(min(min(top_l, min(top_r, top)), left), right)
                if (10 * cur) & U32 > (th0 * local) & U32:
                    status = 1
        aura[i] = status
    return aura


def is_avc_partitioning(rec, jb, scene, high_intra, aura, complete, i):
    """IsAvcPartitioningMode (:1232) -> the number of the deciding clause, 0 for EB_FALSE"""
    if jb["cls"] <= 1:
        return 0
    sp = rec["sbo_pic"][0]
    if sp["high_dark_low_light_area_density"] and jb["layer"] > 0 and rec["detect"]["sharp_edge"][i] and not rec["sbo_lcu"]["similar_colocated_all_layers"][i]:
        return 1
    if scene == 0 and int(sp["grass_percentage"]) > 60 and aura[i] == 1 and high_intra == 0 and complete[i]:
        return 2
    if rec["pic_detect"][0]["logo_pic"] and rec["detect"]["edge_block_num"][i]:
        return 3
    if rec["stationary_edge"] is not None and rec["stationary_edge"][i] > 0:
        return 4
    if rec["sbo_lcu"]["complex_lcu"][i] == 2:
        return 5
    return 0


def target_budget(n, jb, sens):
    """SetTargetBudgetOq (:1079)"""
    enc, cls, layer, ref, pan_tilt = jb["enc_mode"], jb["cls"], jb["layer"], jb["ref"], jb["pan"] or jb["tilt"]
    adp = (n * 127 if sens == 2 else n * 125 if sens == 1 else n * 121) if layer == 0 else (n * 110 if sens == 2 else n * 100) if ref else n * 100
    plain = n * 129 if layer == 0 else n * 110 if ref else n * 109
    if enc <= 5:
        if cls <= 1:
            return n * 155 if layer == 0 else (n * 152 if pan_tilt else n * 150) if ref else (n * 152 if pan_tilt else n * 145)
        if cls <= 2:
            return n * 155 if layer == 0 else n * 138 if ref else n * 134
        if enc <= 3:
            return plain
        return n * 155 if layer == 0 else n * 125 if ref else n * 121
    if enc <= 7:
        return plain
    if enc <= 8:
        return adp if cls == 3 else plain
    return adp


def default_segments(n, jb, sens, budget):
    """DeriveDefaultSegments (:942) -> (numberOfSegments, the interval modes); scoreTh[k] = (k + 1) * 100 / numberOfSegments for k < numberOfSegments - 1"""
    if jb["layer"] == 0:
        if sens and budget >= n * 123:
            return (2, (R.LCU_BDP, R.LCU_FULL84)) if budget > n * 129 else (2, (R.LCU_LIGHT_BDP, R.LCU_BDP))
        if budget > n * 129:
            return 2, (R.LCU_BDP, R.LCU_FULL84)
        if budget > n * 110:
            return 4, (R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_LIGHT_BDP, R.LCU_BDP)
        return 5, (R.LCU_PRED_OPEN_LOOP_1_NFL, R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_LIGHT_BDP, R.LCU_BDP)
    if budget > n * 120:
        return 6, (R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_OPEN_LOOP, R.LCU_LIGHT_BDP, R.LCU_BDP, R.LCU_FULL85)
    if budget > n * 115:
        return 5, (R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_OPEN_LOOP, R.LCU_LIGHT_BDP, R.LCU_BDP)
    if budget > n * 110:
        return 4, (R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_OPEN_LOOP, R.LCU_LIGHT_BDP)
    return 4, (R.LCU_PRED_OPEN_LOOP_1_NFL, R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_OPEN_LOOP)


def lcu_scores(w, h, rec, jb):
    """DeriveLcuScore (:1596), the P / B arm"""
    wl, hl, col, row, complete, edge = R.geometry(w, h)
    valid = R.unit_validity(w, h)
    sp, sl, dist = rec["sbo_pic"][0], rec["sbo_lcu"], rec["me"]["pu"]["distortion"][:, :, 0]
    cmin, cmax = int(sp["inter_complexity_min"][0]), int(sp["inter_complexity_max"][0])
    nm_avg = int(sp["non_moving_index_average"])
    scores = []
    for i in range(len(col)):
        if not complete[i]:
            total, count = 0, 0
            for k in range(21, 85):                                   # raster order of the 8x8 units
                if valid[i][RASTER_TO_MD[k]]:
                    total, count = (total + int(dist[i, k])) & U32, count + 1
            if count:
                v = ((total // count) * 64) & U32
                total = cmin if v < cmin else cmax if v > cmax else v
            scores.append(total)
            continue
        s = int(dist[i, 0])
        nmi = int(sl["non_moving_index"][i])
        if sl["failing_motion"][i]:
            s = cmax
        elif edge[i] and nmi != 0xFF and nm_avg != 0xFF and nmi >= 10 and (nmi >= nm_avg or nm_avg > 25) and jb["cls"] == 3:
            s = (s + ((((cmax - s) & U32) * 75) & U32) // 100) & U32
        else:
            down = lambda v: (v - ((((v - cmin) & U32) * 50) & U32) // 100) & U32  # noqa: E731
            up = lambda v: (v + ((((cmax - v) & U32) * 50) & U32) // 100) & U32    # noqa: E731
            if nmi == 30 and int(rec["stats"]["variance"][i, 0]) > 100 and jb["fr30"]:
                s = down(s)
            dark_lcu = int(rec["stats"]["y_mean"][i, 0]) < 25
            if jb["cls"] == 3:
                if int(sp["black_area_percentage"]) > 25:
                    s = down(s) if dark_lcu else up(s)
            else:
                s = down(s) if dark_lcu else up(s)
        scores.append(s)
    return scores


def outlier_removal(scores, complete, lo, hi):
    """PerformOutlierRemoval (:1736) -> (lcuMinScore, lcuMaxScore)"""
    sub = ((hi - lo) & U32) // 10
    hist, processed = [0] * 10, 0
    for s, c in zip(scores, complete):
        if not c:
            continue
        processed += 1
        v = (s + lo) & U32
        for k in range(10):
            if v < ((k + 1) * sub + lo) & U32:
                hist[k] += 1
                break
    if processed:
        hist = [0 if (c * 100) // processed < 2 else c for c in hist]
    for k in range(10):
        if hist[k]:
            lo = (lo + k * sub) & U32
            break
    for k in range(9, -1, -1):
        if hist[k]:
            hi = (hi - (9 - k) * sub) & U32
            break
    return lo, hi


def lcu_md_modes(w, h, rec, jb, scene, high_intra, aura):
    """DeriveLcuMdMode (:1826) -> (lcu_md_mode, avc clause, score, cost per LCU; the ADP fields of the picture record)"""
    wl, hl, col, row, complete, edge = R.geometry(w, h)
    n = wl * hl
    sp, noise = rec["sbo_pic"][0], int(rec["noise_pic"][0]["pic_noise_class"])
    # ConfigureAdp
    lum = False
    if jb["ref"]:
        th = ADP_LUMINOSITY_CHANGE_TH[jb["hier"]][jb["layer"]]
        lum = abs(jb["avg_int"] - jb["ref_int0"]) >= th or (jb["slice_type"] == R.B and abs(jb["avg_int"] - jb["ref_int1"]) >= th)
    nm_avg, sens = int(sp["non_moving_index_average"]), 0
    if nm_avg != 0xFF and nm_avg < 30:
        if noise > 3 or sp["high_dark_low_light_area_density"] or lum:
            sens = 2
        elif nm_avg >= 15 and noise == 3:
            sens = 1
    budget = target_budget(n, jb, sens)
    nseg, modes = default_segments(n, jb, sens, budget)
    th = [-1] * 7
    for k in range(nseg - 1):
        th[k] = _s8(((k + 1) * 100) // nseg)
    interval = [COST[m] for m in modes] + [0] * (7 - nseg)
    clause = [is_avc_partitioning(rec, jb, scene, high_intra, aura, complete, i) for i in range(n)]
    avc = [c != 0 for c in clause]
    # ComputeRefinementCost
    avc_cost = sum(138 if a else interval[0] for a in avc)
    light_cost = sum(122 if a else interval[0] for a in avc)
    if avc_cost <= budget and (budget > 123 * n or jb["layer"] == 0 or (jb["cls"] < 3 and jb["ref"])):
        mode = 2
    elif light_cost <= budget and jb["layer"] > 0:
        mode = 1
    else:
        mode = 0
    scores = lcu_scores(w, h, rec, jb)
    lo, hi = outlier_removal(scores, complete, min(scores), max(scores))
    # DeriveOptimalBudgetPerLcu / SetLcuBudget
    predicted, deviation, initial, final, iteration = U32, 1000, 2, 2, 0      # TBD_SHOOTING
    cost = [0] * n
    while deviation != 0 and initial == final and iteration <= 100:
        initial = 0 if predicted < budget else 1                             # UNDER_SHOOTING / OVER_SHOOTING
        predicted = 0
        for i in range(n):
            if mode == 2 and avc[i]:
                cost[i] = 138
            elif mode == 1 and avc[i]:
                cost[i] = 122
            else:
                scores[i] = lo if scores[i] < lo else hi if scores[i] > hi else scores[i]
                to_min, span = (scores[i] - lo) & U32, (hi - lo) & U32
                for k in range(7):
                    if k == 6 or (to_min <= ((span * (th[k] & U32)) & U32) // 100 and th[k] != 0) or nseg == k + 1 or th[k + 1] == 100:
                        cost[i] = interval[k]
                        break
                if avc[i]:
                    if cost[i] > 138:
                        cost[i] = 138
                    elif cost[i] > 122 and jb["layer"] > 0:
                        cost[i] = 122
            predicted = (predicted + cost[i]) & U32
        # ABS((EB_S32)(predictedCost - budget)) * 1000 (:1522) is a SIGNED product: beyond 2^31 the reference's behaviour is not defined, and nothing is restated
        # there.  predictedCost and budget are both at most 155 a LCU, so the product stays below 2^31 for every picture of up to 13,854 LCUs (a 4K picture has
        # 2,040); the inputs of tests/mdc_records.py are far inside that, which the assertion holds the restatement to
        assert abs(_s32(predicted - budget)) * 1000 < 1 << 31, (predicted, budget)
        deviation = (abs(_s32(predicted - budget)) * 1000) // budget
        if predicted < budget:
            for k in range(5):
                th[k] = _s8(max(th[k] - 1, 0))
            final = 0
        else:
            for k in range(5):
                th[k] = 0 if th[k] == 0 else _s8(min(th[k] + 1, 100))
            final = 1
        if iteration == 0:
            initial = final
        iteration += 1
    # DeriveSearchMethod: the order of the equality tests (:1360-1392)
    order = (R.LCU_PRED_OPEN_LOOP_1_NFL, R.LCU_PRED_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_OPEN_LOOP, R.LCU_LIGHT_BDP, R.LCU_BDP, R.LCU_AVC, R.LCU_LIGHT_AVC)
    md_mode = []
    for c in cost:
        md_mode.append(next((m for m in order if COST[m] == c), R.LCU_FULL84 if jb["layer"] == 0 else R.LCU_FULL85))
    bdp = any(m in (R.LCU_LIGHT_BDP, R.LCU_BDP) for m in md_mode)
    md = any(m not in (R.LCU_LIGHT_BDP, R.LCU_BDP) for m in md_mode)
    pic = dict(adp_depth_sensitive_picture_class=sens, adp_refinement_mode=mode, number_of_segments=nseg, budget=budget, predicted_cost=predicted,
               lcu_min_score=lo, lcu_max_score=hi, score_th=th, interval_cost=interval, iterations=iteration, bdp_present=int(bdp), md_present=int(md))
    return md_mode, clause, scores, cost, pic


def forward_fixed(valid, mode):
    """Forward85 / 84 / 8x816x16 / 16x16CuToModeDecisionLCU (:370-704) -> [(leafIndex, splitFlag)]"""
    first = {R.LCU_FULL85: 0, R.LCU_FULL84: 1, R.LCU_AVC: 2, R.LCU_LIGHT_AVC: 2}[mode]
    stop = 2 if mode == R.LCU_LIGHT_AVC else 3
    out, cu = [], 0
    while cu < 85:
        split, depth = True, MD_SCAN[cu][0]
        if valid[cu]:
            if depth >= first:
                split = depth < stop
                out.append((cu, int(split)))
        cu += 1 if split else DEPTH_OFFSET[depth]
    return out


def mdc_refinement(selected, stop, cu, depth, level, lowest):
    """EbHevcMdcRefinement (Codec/EbModeDecisionConfiguration.c:82)"""
    if level & P_:
        if lowest == P_:
            stop[cu] = True
    else:
        selected[cu] = False
    if level & Pp1 and depth < 3 and cu < 81:
        for q in range(4):
            selected[cu + 1 + q * DEPTH_OFFSET[depth + 1]] = True
            if lowest == Pp1:
                stop[cu + 1 + q * DEPTH_OFFSET[depth + 1]] = True
    if level & Pp2 and depth < 2 and cu < 65:
        for a in range(4):
            for b in range(4):
                at = cu + 1 + a * DEPTH_OFFSET[depth + 1] + 1 + b * DEPTH_OFFSET[depth + 2]
                selected[at] = True
                if lowest == Pp2:
                    stop[at] = True
    if level & Pp3 and depth == 0:
        for at in range(85):
            if MD_SCAN[at][0] == 3:
                selected[at] = True
                if lowest == Pp3:
                    stop[at] = True
    if level & Pm1 and depth > 0:
        selected[cu - 1 - PARENT_CU_INDEX[cu]] = True
        if lowest == Pm1:
            stop[cu - 1 - PARENT_CU_INDEX[cu]] = True
    if level & Pm2:
        for at in ((0,) if depth == 2 else (1, 22, 43, 64) if depth == 3 else ()):
            selected[at] = True
            if lowest == Pm2:
                stop[at] = True
    if level & Pm3 and depth == 3:
        selected[0] = True
        if lowest == Pm2:                                                 # as written (:232)
            stop[0] = True


def early_mode_decision(valid, pu, jb, md_mode, lam, split_bits):
    """EarlyModeDecisionLcu (:1059) of a P / B picture under PICT_LCU_SWITCH -> ([(leafIndex, splitFlag)], pred64)"""
    start, end = (1 if jb["layer"] == 0 else 0), 2
    cost, early_split = [0] * 85, [False] * 85                           # units outside the picture are never read
    rate0, rate1 = (lam * split_bits[0] + (1 << 22)) >> 23, (lam * split_bits[1] + (1 << 22)) >> 23
    g8, g16 = 0, 0
    # EbHevcPredictionPartitionLoop (:903)
    for cu in range(85):
        depth, size, x, y, raster = MD_SCAN[cu]
        if not valid[cu]:
            continue
        early_split[cu] = depth < end
        if not (start <= depth <= end):
            cost[cu] = U32
            continue
        u = pu[raster]
        cost[cu] = ((int(u["distortion"][0]) << 8) & U32) + ((lam * inter_cu_rate(int(u["direction"][0]), u["mv"]) + (1 << 22)) >> 23)
        g8 = INCREMENTAL_COUNT[raster] if depth == 2 else 0              # endDepth == 2 (:1032)
        # EbHevcMdcInterDepthDecision (:715); the 8x8 stage never runs: depth 3 is outside the range
        two = one = cu
        if (x >> 3) & 1 and (y >> 3) & 1:
            raise AssertionError("an 8x8 unit in the P / B range")
        if ((MD_SCAN[two][2] >> 3) & 2) == 2 and ((MD_SCAN[two][3] >> 3) & 2) == 2 and g8 == 4:
            g8, g16 = 0, g16 + 1
            left = two - 5
            top = left - 5
            top_left = top - 5
            one = top_left - 1
            if MD_SCAN[one][0] == 1:
                n_cost = cost[one] + rate0
                n1_cost = cost[two] + cost[left] + cost[top] + cost[top_left] + rate1
                if n_cost <= n1_cost:
                    early_split[one], cost[one] = False, n_cost
                else:
                    cost[one] = n1_cost
        if ((MD_SCAN[one][2] >> 3) & 4) == 4 and ((MD_SCAN[one][3] >> 3) & 4) == 4 and g16 == 4:
            g16 = 0
            left = one - 21
            top = left - 21
            top_left = top - 21
            zero = top_left - 1
            if MD_SCAN[zero][0] == 0:
                n_cost = cost[zero] + rate0
                n1_cost = cost[one] + cost[left] + cost[top] + cost[top_left] + rate1
                if n_cost <= n1_cost:
                    early_split[zero] = False
    # EbHevcRefinementPredictionLoop (:436)
    selected, stop = [False] * 85, [False] * 85
    pred64, cu = 0, 0
    while cu < 85:
        if valid[cu] and not early_split[cu]:
            selected[cu] = True
            pred64 = 1 if cu == 0 else pred64
            depth = MD_SCAN[cu][0]
            if md_mode in (R.LCU_PRED_OPEN_LOOP, R.LCU_PRED_OPEN_LOOP_1_NFL):
                level = P_
            elif md_mode == R.LCU_OPEN_LOOP:
                level = NDP_NREF[jb["layer"]][depth]
            else:
                level = NDP_FAST[jb["layer"]][depth]
            if jb["cu8"] == 1:
                if level & Pp1 and depth == 2:
                    level -= Pp1
                elif level & Pp2 and depth == 1:
                    level -= Pp2
                elif level & Pp3 and depth == 0:
                    level -= Pp3
            lowest = next((b for b in (Pp3, Pp2, Pp1, P_, Pm1, Pm2, Pm3) if level & b), 0)
            mdc_refinement(selected, stop, cu, depth, level, lowest)
            cu += DEPTH_OFFSET[depth]
        else:
            cu += 1
    # EbHevcForwardCuToModeDecision (:586)
    out, cu = [], 0
    while cu < 85:
        split, depth = True, MD_SCAN[cu][0]
        if valid[cu]:
            if depth < 3:
                if stop[cu]:
                    split = False
                    out.append((cu, 0))
                elif selected[cu]:
                    out.append((cu, 1))
            else:
                split = False
                out.append((cu, 0))
        cu += 1 if split else DEPTH_OFFSET[depth]
    return out, pred64


def md_config(w, h, rec, jb, lam, split_bits):
    """rec: the records of mdc_records.make_inputs; jb: the job's parameters; lam, split_bits: the picture's SAD lambda and splitFlagBits[0], [3].
    -> (MDC_LCU_DTYPE[lcus], MDC_PIC_DTYPE record, the deciding clause of IsAvcPartitioningMode per LCU)"""
    wl, hl, col, row, complete, edge = R.geometry(w, h)
    n = wl * hl
    valid = R.unit_validity(w, h)
    lcu, pic = np.zeros(n, R.MDC_LCU_DTYPE), np.zeros(1, R.MDC_PIC_DTYPE)[0]
    scene, adjust, high_intra, offset = picture_signals(rec, jb)
    pic["scene_characteristic_id"], pic["adjust_min_qp"], pic["high_intra_selection"] = scene, adjust, high_intra
    pic["slice_cb_qp_offset"], pic["slice_cr_qp_offset"], pic["average_qp"] = offset, offset, jb["qp"]
    aura = aura_detection(w, h, rec, jb)
    lcu["aura_status"] = aura
    clause = [0] * n
    mode = jb["depth_mode"]
    if mode == R.PICT_LCU_SWITCH:
        md_mode, clause, scores, cost, adp = lcu_md_modes(w, h, rec, jb, scene, high_intra, aura)
        for k, v in adp.items():
            pic[k] = v
        lcu["lcu_md_mode"], lcu["lcu_score"], lcu["lcu_cost"], lcu["avc_partitioning"] = md_mode, scores, cost, [c != 0 for c in clause]
    for i in range(n):
        if mode == R.PICT_LCU_SWITCH:
            m = md_mode[i]
            if m in (R.LCU_BDP, R.LCU_LIGHT_BDP):
                leaves = []
            elif m in (R.LCU_FULL85, R.LCU_FULL84, R.LCU_AVC, R.LCU_LIGHT_AVC):
                leaves = forward_fixed(valid[i], m)
            else:
                leaves, lcu["pred64"][i] = early_mode_decision(valid[i], rec["me"]["pu"][i], jb, m, lam, split_bits)
        elif mode in (R.PICT_FULL85, R.PICT_FULL84):
            leaves = forward_fixed(valid[i], R.LCU_FULL85 if mode == R.PICT_FULL85 else R.LCU_FULL84)
        else:
            leaves = []
        lcu["leaf_count"][i] = len(leaves)
        for k, (index, split) in enumerate(leaves):
            lcu["leaf_index"][i, k], lcu["leaf_split"][i, k] = index, split
    return lcu, pic, clause
