"""Plain-Python restatement of the initial rate control's look-ahead stage with the checks in front of it and the stationary-edge stage behind it (the records
of tests/irc_records.py), written from the text of the reference: StationaryEdgeOverUpdateOverTimeLcuPart1 / Part2 (Codec/EbMotionEstimationProcess.c:502,
:554), EbHevcDetectGlobalMotion, EbHevcUpdateGlobalMotionDetectionOverTime, EbHevcUpdateMotionFieldUniformityOverTime, EbHevcStationaryEdgeCountLcu,
UpdateHomogeneityOverTime (Codec/EbInitialRateControlProcess.c:218, :441, :598, :394, :646), the branches of InitialRateControlKernel that call them (:941-1062)
and StationaryEdgeOverUpdateOverTimeLcu (Codec/EbSourceBasedOperationsProcess.c:1142).  Loops run in the reference's order, every width is spelled out, nothing
is repaired.  Pinned on the reference's own results by tests/test_irc_cpu.py."""
import numpy as np

import irc_records as R

U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
# [hierarchicalLevels][temporalLayerIndex] (Codec/EbDefinitions.h:1184); entries the reference's initialisers leave out are 0
GLOBAL_MOTION_THRESHOLD = ((2, 0, 0, 0, 0, 0), (4, 2, 0, 0, 0, 0), (8, 4, 2, 0, 0, 0), (16, 8, 4, 2, 0, 0), (32, 16, 8, 4, 2, 0), (64, 32, 16, 8, 4, 2))
LOW_AMPLITUDE_TH, PAN_LCU_PERCENTAGE = 64, 75


def _s32(v):
    v &= U32
    return v - (1 << 32) if v & 0x80000000 else v


def _u64_of_int(v):
    """an int converted to EB_U64"""
    return v & U64


# ---------------------------------------------------------------- the queue ----------------------------------------------------------------

def _next(index):
    return 0 if index == R.QUEUE_DEPTH - 1 else index + 1


def frames_in_sw(queue, head, pics, lad):
    """framesInSw of the picture at the head (:941-959): the entries counted from the head until the end-of-sequence picture has been counted, lookAheadDistance
    + 1 at most; None where the window is not full yet (moveSlideWondowFlag false)"""
    index, eos, count = head, pics[queue[head]]["eos"] if queue[head] is not None else 0, 0
    while not eos and index <= head + lad:
        count += 1
        entry = queue[index - R.QUEUE_DEPTH if index > R.QUEUE_DEPTH - 1 else index]
        if entry is None:
            return None
        eos = pics[entry]["eos"]
        index += 1
    return count


def window_lists(queue, head, pics, frames, lad, period):
    """the queue state -> what the device job takes: look_ahead, frames_to_check and the three lists, as indices into `pics`.
    queue: QUEUE_DEPTH entries, an index into pics or None; head: initialRateControlReorderQueueHeadIndex; frames: framesInSw of the picture at the head"""
    me = pics[queue[head]]
    look_ahead = int(not me["eos"] and lad != 0)
    if not look_ahead:
        return dict(look_ahead=0, frames_to_check=1, edge=[], hom=[], pan=[])
    to_check = min(min((period << 1) + 1, frames), lad)                       # noFramesToCheck (:611, :679)
    # EbHevcUpdateGlobalMotionDetectionOverTime: the first MIN(8, framesInSw) entries FROM THE HEAD
    pan, index = [], head
    for _ in range(min(8, frames)):
        if pics[queue[index]]["slice_type"] != R.I:
            pan.append(queue[index])
        index = _next(index)
    # EbHevcUpdateMotionFieldUniformityOverTime (:614): from the head - but from index 0 when the head is the last index
    edge, index = [], 0 if head == R.QUEUE_DEPTH - 1 else head
    for _ in range(to_check - 1):
        t = pics[queue[index]]
        if t["eos"]:
            break
        if (t["poc"] & 3) == 0:
            edge.append(queue[index])
        index = _next(index)
    # UpdateHomogeneityOverTime (:682): the same start
    hom, index = [], 0 if head == R.QUEUE_DEPTH - 1 else head
    for _ in range(to_check - 1):
        t = pics[queue[index]]
        if t["scene"] or t["eos"]:
            break
        hom.append(queue[index])
        index = _next(index)
    return dict(look_ahead=1, frames_to_check=to_check, edge=edge, hom=hom, pan=pan)


def sequence_lists(seq):
    """the lists of every picture of a sequence of irc_records.sequence, each taken when the picture stands at the head with all later pictures in the queue"""
    pics = seq["pics"]
    queue = [None] * R.QUEUE_DEPTH
    for k in range(len(pics)):
        queue[(seq["head0"] + k) % R.QUEUE_DEPTH] = k
    out, head = [], seq["head0"] % R.QUEUE_DEPTH
    for k in range(len(pics)):
        if pics[k]["eos"]:
            frames = 1      # :936: the loop does not run; the picture leaves with framesInSw 0 -> no window either way
        else:
            frames = frames_in_sw(queue, head, pics, seq["lad"])
            assert frames is not None
        out.append(window_lists(queue, head, pics, frames, seq["lad"], seq["period"]))
        queue[head] = None
        head = _next(head)
    return out


# ---------------------------------------------------------------- per picture ----------------------------------------------------------------

def lcu_checks(w, h, cls, rec, p, look_ahead):
    """Part1 and, with look_ahead, Part2 of every LCU -> CHECKS_DTYPE[lcus]; without Part2 the 0 of the EB_MEMSET in EdgeDetectionMeanLumaChroma16x16"""
    wl, hl, col, row, complete, logo = R.geometry(w, h, cls)
    out = np.zeros(wl * hl, R.CHECKS_DTYPE)
    low_sad_th = 5 if cls < 2 else 2                                        # inputResolution < INPUT_SIZE_1080p_RANGE
    for n in range(wl * hl):
        if logo[n] and complete[n]:
            x = y = 0
            if p["layer"] > 0:
                x, y = (int(v) for v in rec["me"]["pu"]["mv"][n, 0, :2])
            low_motion = True if p["layer"] == 0 else abs(x) < 16 and abs(y) < 16
            var = [int(v) for v in rec["stats"]["variance"][n, 1:5]]                 # EB_U64
            average = sum(var) >> 2
            products = [_s32(_s32(v - average) * _s32(v - average)) for v in var]    # (EB_S32) * (EB_S32): int
            total = _s32(_s32(_s32(products[0] + products[1]) + products[2]) + products[3])
            var_of_var = _u64_of_int(total) >> 2
            out["check1"][n] = 0 if var_of_var <= 50000 or not low_motion else 1
            out["pm_check1"][n] = 0 if var_of_var <= 1000 else 1
        if look_ahead:
            if logo[n] and complete[n]:
                dist = int(rec["me"]["pu"]["distortion"][n, 0, 0]) if p["slice_type"] == R.B else 0
                low_sad = p["slice_type"] == R.B and dist < 64 * 64 * low_sad_th
                out["low_dist_logo"][n] = 1 if low_sad else 0
            out["check2"][n] = 1                                                  # the function's last line (:591)
    return out


def _pan(th, xc, yc, xk, yk):
    return yc < LOW_AMPLITUDE_TH and yk < LOW_AMPLITUDE_TH and _s32(xc * xk) > 0 and abs(xc) >= th and abs(xk) >= th and abs(xc - xk) < LOW_AMPLITUDE_TH


def _pan_high(th, xc, xk):
    return _s32(xc * xk) > 0 and abs(xc) >= th and abs(xk) >= th and abs(xc - xk) < LOW_AMPLITUDE_TH


def global_motion(w, h, cls, rec, p):
    """EbHevcMeBasedGlobalMotionDetection -> (MOTION_DTYPE record, the vote byte of every LCU)"""
    wl, hl, col, row, complete, logo = R.geometry(w, h, cls)
    m, votes = np.zeros((), R.MOTION_DTYPE), np.zeros(wl * hl, np.uint8)
    if p["slice_type"] == R.I:
        return m, votes
    th = GLOBAL_MOTION_THRESHOLD[p["hier"]][p["layer"]]
    mv = rec["me"]["pu"]["mv"][:, 0, :2].astype(int)
    checked = pan = tilt = pan_high = tilt_high = 0
    for n in range(wl * hl):
        if not complete[n]:
            continue
        ox, oy = int(col[n]) * 64, int(row[n]) * 64
        xc, yc = mv[n]
        left = (0, 0) if ox == 0 else mv[n - 1]
        top = (0, 0) if oy == 0 else mv[n - wl]
        right = (0, 0) if ox + 128 > w else mv[n + 1]
        bottom = (0, 0) if oy + 128 > h else mv[n + wl]
        checked += 1
        cand = (left, top, right, bottom)
        v = 0
        if any(_pan(th, xc, yc, xk, yk) for xk, yk in cand):
            pan, v = pan + 1, v | 1
        if any(_pan(th, yc, xc, yk, xk) for xk, yk in cand):                    # CheckMvForTilt: the same test with x and y exchanged
            tilt, v = tilt + 1, v | 2
        if any(_pan_high(th, xc, xk) for xk, yk in cand):
            pan_high, v = pan_high + 1, v | 4
        if any(_pan_high(th, yc, yk) for xk, yk in cand):
            tilt_high, v = tilt_high + 1, v | 8
        votes[n] = v
    m["total_checked_lcus"], m["total_pan_lcus"], m["total_tilt_lcus"], m["total_pan_high_amp_lcus"], m["total_tilt_high_amp_lcus"] = checked, pan, tilt, pan_high, tilt_high
    if checked > 0:
        m["is_pan_raw"] = (pan * 100 & U32) // checked > PAN_LCU_PERCENTAGE
        m["is_tilt_raw"] = (tilt * 100 & U32) // checked > PAN_LCU_PERCENTAGE
    return m, votes


def pan_over_time(p, own_motion, pan_motion, look_ahead):
    """-> is_pan, is_tilt as the picture leaves the stage (:1012-1026)"""
    if not look_ahead:
        return int(own_motion["is_pan_raw"]), int(own_motion["is_tilt_raw"])
    total_pan = sum(int(m["is_pan_raw"]) == 1 for m in pan_motion)
    checked = len(pan_motion)
    is_pan = 0
    if checked and p["slice_type"] != R.I and total_pan * 100 // checked > 75:
        is_pan = 1
    return is_pan, 0                                                            # isTilt = EB_FALSE (:488), never set again


def edge_counts(own, edge_checks, edge_detect):
    """EbHevcStationaryEdgeCountLcu over the entries that count -> similarEdgeCount [lcus][16], pmSimilarEdgeCount [lcus][16]; check1 / pm_check1 carry
    potentialLogoLcu && isCompleteLcu (Part1 sets them nowhere else)"""
    n = own.size
    count, pm_count = np.zeros((n, 16), np.uint8), np.zeros((n, 16), np.uint8)
    for checks, detect in zip(edge_checks, edge_detect):
        for i in range(n):
            if own["check1"][i] and own["check2"][i] and checks["check1"][i]:
                for k in range(16):
                    count[i, k] += int(detect["edge_cu"][i]) >> k & 1
            if own["pm_check1"][i] and own["check2"][i] and checks["pm_check1"][i]:
                for k in range(16):
                    pm_count[i, k] += int(detect["edge_cu"][i]) >> k & 1
    return count, pm_count


def homogeneity(n, hom_stats, look_ahead, to_check):
    """UpdateHomogeneityOverTime / ResetHomogeneityStructures -> lcuVarianceOfVarianceOverTime [lcus], isLcuHomogeneousOverTime [lcus]"""
    var_of_var, homogeneous = np.full(n, U64, np.uint64), np.zeros(n, np.uint8)
    if not look_ahead:
        return var_of_var, homogeneous
    for i in range(n):
        mean_sqr = mean = 0                                                     # EB_U64
        for st in hom_stats:
            v = int(st["variance"][i, 0])
            mean_sqr = (mean_sqr + _u64_of_int(_s32(v * v))) & U64              # the int product of two promoted EB_U16
            mean = (mean + v) & U64
        if to_check == 1:
            mean_sqr = mean = 0
        else:
            mean_sqr, mean = mean_sqr // (to_check - 1), mean // (to_check - 1)
        vv = (mean_sqr - mean * mean) & U64
        var_of_var[i] = vv
        homogeneous[i] = vv <= 64 * 64
    return var_of_var, homogeneous


def clear_isolated_loop(flag, eligible, wl, hl):
    """pass (a) as written (:1197-1244): in place, in raster order"""
    flag = flag.copy()
    for n in range(wl * hl):
        x, y = n % wl, n // wl
        if eligible[n]:
            count = 0
            for v in range(-1 if y > 0 else 0, (1 if y < hl - 1 else 0) + 1):
                for c in range(-1 if x > 0 else 0, (1 if x < wl - 1 else 0) + 1):
                    count += flag[n + v * wl + c] == 1
            if count == 1:
                flag[n] = 0
    return flag


def clear_isolated_gather(flag, wl, hl):
    """pass (a) as the device runs it: an LCU is cleared when its flag is 1 and none of its eight neighbours' flags was 1 before the pass"""
    out = flag.copy()
    for n in range(wl * hl):
        x, y = n % wl, n // wl
        if flag[n] == 1:
            near = 0
            for v in range(-1 if y > 0 else 0, (1 if y < hl - 1 else 0) + 1):
                for c in range(-1 if x > 0 else 0, (1 if x < wl - 1 else 0) + 1):
                    near += (v != 0 or c != 0) and flag[n + v * wl + c] == 1
            if near == 0:
                out[n] = 0
    return out


def _spread(flag, gate, wl, hl, want, more_than, value):
    """passes (b) and (c) as written (:1258-1317, :1330-1389): in place, in raster order"""
    for n in range(wl * hl):
        x, y = n % wl, n // wl
        if flag[n] == 0 and gate[n]:
            count = 0
            for v in range(-1 if y > 0 else 0, (1 if y < hl - 1 else 0) + 1):
                for c in range(-1 if x > 0 else 0, (1 if x < wl - 1 else 0) + 1):
                    count += flag[n + v * wl + c] == want
            if count > more_than:
                flag[n] = value


def stationary_edge(w, h, cls, own, count, pm_count, look_ahead, to_check, trace=None):
    """StationaryEdgeOverUpdateOverTimeLcu with totalCheckedPictures = noFramesToCheck -> stationaryEdgeOverTimeFlag [lcus], pmStationaryEdgeOverTimeFlag [lcus]
    (0 without look_ahead: the memset's).  trace: a dict that receives the planes before and after pass (a)"""
    wl, hl, col, row, complete, logo = R.geometry(w, h, cls)
    n = wl * hl
    flag, pm_flag = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if not look_ahead:
        return flag, pm_flag
    slide_th = (to_check // 4 - 1) & U32                                        # EB_U32
    eligible = logo & complete & (own["check1"] != 0) & (own["check2"] != 0)
    pm_eligible = logo & complete & (own["pm_check1"] != 0) & (own["check2"] != 0)
    for i in range(n):
        if eligible[i]:
            flag[i] = sum(int(c) > slide_th for c in count[i]) >= 4
        if pm_eligible[i]:
            pm_flag[i] = sum(int(c) > slide_th for c in pm_count[i]) >= 4
    if trace is not None:
        trace["before"], trace["pm_before"] = flag.copy(), pm_flag.copy()
    flag, pm_flag = clear_isolated_loop(flag, eligible, wl, hl), clear_isolated_loop(pm_flag, pm_eligible, wl, hl)
    if trace is not None:
        trace["after"], trace["pm_after"] = flag.copy(), pm_flag.copy()
    gate = logo & ((own["check2"] != 0) | ~complete)                            # the same for both planes (:1267, :1339)
    _spread(flag, gate, wl, hl, 1, 0, 2)
    _spread(flag, gate, wl, hl, 2, 3, 3)
    _spread(pm_flag, gate, wl, hl, 1, 0, 2)
    _spread(pm_flag, gate, wl, hl, 2, 3, 3)
    return flag, pm_flag


# ---------------------------------------------------------------- a sequence ----------------------------------------------------------------

def initial_rc(w, h, cls, seq, recs, lists=None, trace=None, only=None):
    """every picture of a sequence -> dict of arrays, picture k first: checks [n][lcus], motion [n], lcu [n][lcus], stationary_edge / pm_stationary_edge
    [n][lcus], picture [n].  lists: sequence_lists(seq) where the caller has them.  trace: a list that receives one dict a picture (stationary_edge's).
    only: the pictures whose look-ahead stage is wanted - the others keep their checks, motion record and votes, the rest of their records stays 0"""
    pics = seq["pics"]
    lists = lists or sequence_lists(seq)
    count, n = len(pics), ((w + 63) // 64) * ((h + 63) // 64)
    out = dict(checks=np.zeros((count, n), R.CHECKS_DTYPE), motion=np.zeros(count, R.MOTION_DTYPE), lcu=np.zeros((count, n), R.IRC_LCU_DTYPE),
               stationary_edge=np.zeros((count, n), np.uint8), pm_stationary_edge=np.zeros((count, n), np.uint8), picture=np.zeros(count, R.IRC_PIC_DTYPE))
    for k, (p, rec, ls) in enumerate(zip(pics, recs, lists)):
        out["checks"][k] = lcu_checks(w, h, cls, rec, p, ls["look_ahead"])
        out["motion"][k], out["lcu"]["motion_votes"][k] = global_motion(w, h, cls, rec, p)
    for k, (p, rec, ls) in enumerate(zip(pics, recs, lists)):
        if only is not None and k not in only:
            continue
        own, lcu, pr = out["checks"][k], out["lcu"][k], out["picture"][k]
        lcu["similar_edge_count"], lcu["pm_similar_edge_count"] = edge_counts(own, [out["checks"][e] for e in ls["edge"]], [recs[e]["detect"] for e in ls["edge"]])
        lcu["var_of_var_over_time"], lcu["homogeneous_over_time"] = homogeneity(n, [recs[e]["stats"] for e in ls["hom"]], ls["look_ahead"], ls["frames_to_check"])
        tr = {} if trace is not None else None
        out["stationary_edge"][k], out["pm_stationary_edge"][k] = stationary_edge(w, h, cls, own, lcu["similar_edge_count"], lcu["pm_similar_edge_count"],
                                                                                 ls["look_ahead"], ls["frames_to_check"], tr)
        if trace is not None:
            trace.append(tr)
        pr["is_pan"], pr["is_tilt"] = pan_over_time(p, out["motion"][k], [out["motion"][e] for e in ls["pan"]], ls["look_ahead"])
        homogeneous = int(lcu["homogeneous_over_time"].sum()) & 0xFFFF            # EB_U16
        pr["homogeneous_lcu_count"], pr["homogeneity_percentage"] = homogeneous, (homogeneous * 100 // n) & 0xFF
        pr["stationary_lcu_count"] = np.bincount(out["stationary_edge"][k], minlength=4)
    return out
