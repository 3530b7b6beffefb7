"""numpy / plain-Python restatement of the batched source-based operations (include/svt_hevc_amd.h "Batched source-based operations"), written from the text of
the reference: SourceBasedOperationsKernel (Codec/EbSourceBasedOperationsProcess.c:1397) and the functions it calls, EbHevcUpdateBeaInfoOverTime
(Codec/EbInitialRateControlProcess.c:519) and DeriveSimilarCollocatedFlag (Codec/EbMotionEstimationProcess.c:462).  Loops run in the reference's order, so the
order-dependent rules (lcuCmplxContrastArray) are simply what the loops leave behind.  Pinned on the reference's own results by tests/test_sbo_cpu.py."""
import numpy as np

from sbo_records import SBO_LCU_DTYPE, SBO_PIC_DTYPE

U32 = 0xFFFFFFFF
THRESHOLD_NOISE = (33, 28, 27, 26, 26, 26)
NSAD_TABLE = (10, 5, 5, 5, 5, 5)
# the parents of 16x16 unit k: its 32x32 (1..4) and the 64x64 (0), as RASTER_SCAN_CU_PARENT_INDEX has them
PARENT_32 = [1 + (k >> 3) * 2 + ((k & 3) >> 1) for k in range(16)]


def _s32(v):
    v &= U32
    return v - (1 << 32) if v & 0x80000000 else v


def _deviation(me, ois):
    """meToOisSadDeviation (:211-212): the difference of two (EB_S32) casts is an int before it becomes EB_S64; the product is EB_S64, the division by the
    EB_U64 SAD unsigned"""
    diff = _s32(_s32(me) - _s32(ois))
    return 0 if ois == 0 or diff < 0 else (diff * 100) // ois


def window_average(zz):
    """EbHevcUpdateBeaInfoOverTime: zz [count][lcus] ZZ_DTYPE -> (zz_cost, non_moving_index) as (EB_U8); EbHevcInitZzCostInfo for an empty window"""
    if len(zz) == 0:
        return None
    count = len(zz)
    return ((zz["zz_cost"].astype(np.uint32).sum(0) // count) & 0xFF).astype(np.uint8), ((zz["non_moving_index"].astype(np.uint32).sum(0) // count) & 0xFF).astype(np.uint8)


def source_ops(w, h, rec, jb, previous_parents=None):
    """rec: the records of sbo_records.make_inputs (ref_stats may be None); jb: the job's parameters.  previous_parents: [lcus][4 kinds][5] - what
    cuStatArray[64x64, 32x32 0..3] of the picture-control-set object held before this picture (None: a fresh object).
    -> (SBO_LCU_DTYPE[lcus], SBO_PIC_DTYPE record, parents after this picture)"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    n_lcu = wl * hl
    st, chroma, det = rec["stats"], rec["chroma"], rec["detect"]
    slice_type, layer = jb["slice_type"], jb["layer"]
    me_d = rec["me"]["pu"]["distortion"][:, :, 0].astype(np.int64) if rec.get("me") is not None else None
    ois_w = rec["ois"]["candidate"][:, :, 0].astype(np.int64) if rec.get("ois") is not None else None
    lcu, pic = np.zeros(n_lcu, SBO_LCU_DTYPE), np.zeros(1, SBO_PIC_DTYPE)[0]
    parents = np.zeros((n_lcu, 4, 5), np.uint8) if previous_parents is None else previous_parents.copy()
    ox, oy = (np.arange(n_lcu) % wl) * 64, (np.arange(n_lcu) // wl) * 64
    complete = (ox + 64 <= w) & (oy + 64 <= h)
    var64, mean64 = st["variance"][:, 0].astype(np.int64), st["y_mean"][:, 0].astype(np.int64)

    avg = window_average(rec["zz"])
    zz_cost, nmi = (np.full(n_lcu, 0xFF, np.uint8),) * 2 if avg is None else avg
    lcu["zz_cost"], lcu["non_moving_index"] = zz_cost, nmi

    # DeriveSimilarCollocatedFlag
    if slice_type != 0 and rec.get("ref_stats") is not None:
        for n in range(n_lcu):
            ref_mean, ref_var = int(rec["ref_stats"]["y_mean"][n, 0]), max(int(rec["ref_stats"]["variance"][n, 0]), 1)
            cur_mean, cur_var = int(mean64[n]), int(var64[n])
            if abs(cur_mean - ref_mean) < 10 and (abs(cur_var * 100 // ref_var - 100) < 10 or abs(cur_var - ref_var) < 10):
                lcu["similar_colocated"][n] = 1 if jb["ref"] else 0
                lcu["similar_colocated_all_layers"][n] = 1

    def ois_dist(n, k):
        return int(ois_w[n, k]) & 0xFFFFF

    def ois_64(n):
        return sum(ois_dist(n, k) for k in range(1, 5))

    # ---- the LCU loop (:1437-1525) ----
    contrast = np.zeros(n_lcu, np.uint8)
    grass_lcus = moving_n = still_n = moving = still = intra = depth1 = 0
    high_contrast = 0
    for n in range(n_lcu):
        contrast[n] = 0                                                  # :1439
        x0, y0 = int(ox[n]), int(oy[n])
        grass_flag = False
        for k in range(16):                                              # GrassSkinLcu
            if x0 + (k & 3) * 16 + 16 > w or y0 + (k >> 2) * 16 + 16 > h:
                continue
            y, cb, cr = int(st["y_mean"][n, 5 + k]), int(chroma["cb_mean"][n, 5 + k]), int(chroma["cr_mean"][n, 5 + k])
            flags = (70 < y < 130 and 80 < cb < 115 and 110 < cr < 135, 52 < y < 130 and 100 < cb < 120 and 135 < cr < 160, cr >= 80 and y > 180,
                     cr >= 127 or cb > 150)
            grass_flag |= flags[0]
            for kind, (name, f) in enumerate(zip(("grass", "skin", "high_luma", "high_chroma"), flags)):
                if f:
                    lcu[name][n] |= 1 << k
                    parents[n, kind, PARENT_32[k]] = parents[n, kind, 0] = 1     # never cleared (:501-517)
        grass_lcus += int(grass_flag)
        if complete[n]:                                                  # SpatialHighContrastClassifier
            high_contrast = 0
            for k in range(16):
                y, cb, cr, var = int(st["y_mean"][n, 5 + k]), int(chroma["cb_mean"][n, 5 + k]), int(chroma["cr_mean"][n, 5 + k]), int(st["variance"][n, 5 + k])
                high_contrast += int(10 < var < 300 and 70 < y < 145 and abs(cb - 140) < 10 and abs(cr - 115) < 15)
        if complete[n] and slice_type != 0 and layer == 0:               # LumaContrastDetectorLcu
            intra += int(ois_64(n) < (int(me_d[n, 0]) & U32))
            depth1 += 1
        if nmi[n] < 10:
            still, still_n = still + int(mean64[n]), still_n + 1
        else:
            moving, moving_n = moving + int(mean64[n]), moving_n + 1
        if slice_type != 0 and complete[n] and not lcu["similar_colocated"][n]:
            dev = [_deviation(int(me_d[n, k]), ois_64(n) if k == 0 else ois_dist(n, k)) for k in range(5)]
            lcu["failing_motion"][n] = any(d > 15 for d in dev)          # FailingMotionLcu
            if layer == 0:
                lcu["uncovered_area"][n] = any(d > 20 for d in dev)      # DetectUncoveredLcu
        if complete[n]:
            high_dist = slice_type == 2 and any((int(me_d[n, 1 + k]) & U32) >> 10 >= NSAD_TABLE[layer] for k in range(4))   # TemporalHighContrastClassifier
            if high_contrast and high_dist:                              # PopulateFromCurrentLcuToNeighborLcus
                if x0 != 0:
                    contrast[n - 1] = 1
                if x0 + 64 < w:
                    contrast[n + 1] = 1
                if y0 != 0:
                    contrast[n - wl] = 1
                if y0 + 64 < h:
                    contrast[n + wl] = 1
                if x0 >= 64 and y0 >= 64:
                    contrast[n - wl - 1] = 1
                if x0 < w - 64 and y0 >= 64:
                    contrast[n - wl + 1] = 1
                if x0 >= 64 and y0 < h - 64:
                    contrast[n + wl - 1] = 1
                if x0 < w - 64 and y0 < h - 64:
                    contrast[n + wl + 1] = 1
    lcu["cmplx_contrast"] = contrast

    # ---- picture-based operations (:1527-1571) ----
    still_mean, moving_mean = (still // still_n if still_n else 0), (moving // moving_n if moving_n else 0)
    pic["dark_background_light_foreground"] = moving_mean > 2 * still_mean and still_mean < 45
    if slice_type != 0 and layer == 0:
        pic["intra_coded_block_probability"] = ((intra * 100 // depth1) if depth1 else 0) & 0xFF
    # DeriveHighDarkAreaDensityFlag: EB_U32 sums and products
    hist = rec["histogram"].reshape(-1, 256).astype(np.int64)
    area = w * h
    pct = lambda count: (((count & U32) * 100) & U32) // area  # noqa: E731
    black25, black40, white = int(hist[:, :25].sum()), int(hist[:, :40].sum()), int(hist[:, 210:].sum())
    pic["high_dark_area_density"] = pct(black25) >= 20
    pic["black_area_percentage"] = pct(black40) & 0xFF
    pic["high_dark_low_light_area_density"] = pct(black40) >= 20 and pct(white) >= 1
    # DetermineIsolatedNonHomogeneousRegionInPicture
    for n in range(n_lcu):
        c, r = n % wl, n // wl
        if not (0 < c < wl - 1 and 0 < r < hl - 1):
            continue
        med = lambda at, need_complete: int(var64[at] <= 50 and (complete[at] or not need_complete))  # noqa: E731
        flat = (med(n - wl - 1, 0) + med(n - wl, 0) + med(n - wl + 1, 1) + med(n + wl - 1, 1) + med(n + wl, 1) + med(n + wl + 1, 1) + med(n + 1, 1) + med(n - 1, 0))
        if flat > 1 and (det["var_of_var_32x32"][n] > 64 * 64).any():
            homog = sum(int(det["homogeneous"][n + v * wl + hh] == 1) for v in (-1, 1) for hh in (-1, 1))
            lcu["isolated_non_homogeneous"][n] = homog >= 2
    # DetermineMorePotentialAuraAreas
    aura = 0
    for n in range(n_lcu):
        if ox[n] < 64 or oy[n] < 64 or ox[n] > w - 64 or oy[n] > h - 64:                                # isEdgeLcu
            continue
        quiet = 0
        if det["edge_block_num"][n] and mean64[n] >= 150:
            for v in (-1, 0, 1):
                for hh in (-1, 0, 1):
                    at = n + v * wl + hh
                    quiet += int(0 <= at < n_lcu and not det["edge_block_num"][at] and nmi[at] < 30)
        aura += int(quiet > 1)
    pic["percentage_of_edge_in_light_background"] = (aura * 100 // n_lcu) & 0xFF
    # DerivePictureActivityStatistics
    count = int(complete.sum())
    pic["complete_lcu_count"] = count
    if count:
        pic["non_moving_index_average"] = int(nmi[complete].astype(np.int64).sum()) // count
        pic["zz_cost_average"] = int(zz_cost[complete].astype(np.int64).sum()) // count
    pic["low_motion_content"] = pic["zz_cost_average"] == 0
    nm_avg = int(pic["non_moving_index_average"])
    # DeriveBlockinessPresentFlag
    for n in range(n_lcu):
        x0, y0 = int(ox[n]), int(oy[n])
        avail = high = int(var64[n] > 100)
        for cond, at in ((x0 != 0, n - 1), (x0 + 64 < w, n + 1), (y0 != 0, n - wl), (y0 + 64 < h, n + wl), (x0 >= 64 and y0 >= 64, n - wl - 1),
                         (x0 < w - 64 and y0 >= 64, n - wl + 1), (x0 >= 64 and y0 < h - 64, n + wl - 1), (x0 < w - 64 and y0 < h - 64, n + wl + 1)):
            if cond:
                avail, high = avail + 1, high + int(var64[at] > 100)
        if high == avail and nmi[n] != 0xFF and nm_avg != 0xFF:
            if nmi[n] == 30 and nm_avg >= 29 and layer > 0 and jb["cls"] == 3:
                lcu["complex_lcu"][n] = 2
            elif nmi[n] == 30 and 23 <= nm_avg < 29:
                lcu["complex_lcu"][n] = 1
    pic["grass_percentage"] = (grass_lcus * 100 // n_lcu) & 0xFF
    # ComplexityClassifier32x32
    if layer >= 1 and slice_type == 2:
        for n in range(n_lcu):
            if complete[n] and any((int(me_d[n, 1 + k]) & U32) >> 10 > THRESHOLD_NOISE[layer] for k in range(4)):
                lcu["cmplx_status"][n] = 4

    if jb["qpm"]:                                                        # QpmGatherStatistics and the picture part (:1585-1660)
        i_min, i_max, i_acc, e_min, e_max, e_acc, leaves = [U32] * 4, [0] * 4, [0] * 4, [U32] * 4, [0] * 4, [0] * 4, [0] * 4

        def gather(depth, o, m):
            i_min[depth], i_max[depth], i_acc[depth] = min(i_min[depth], o), max(i_max[depth], o), (i_acc[depth] + o) & U32
            e_min[depth], e_max[depth], e_acc[depth] = min(e_min[depth], m), max(e_max[depth], m), (e_acc[depth] + m) & U32
            leaves[depth] += 1
        for n in range(n_lcu):
            x0, y0 = int(ox[n]), int(oy[n])
            if not jb["skip"]:
                for b in range(64):
                    bx, by = b & 7, b >> 3
                    if x0 + bx * 8 + 8 > w or y0 + by * 8 + 8 > h:
                        continue
                    word = int(ois_w[n, 21 + b])
                    if jb["cu8"] == 0 and word >> 20 & 1:
                        o = word & 0xFFFFF
                    else:
                        parent = int(ois_w[n, 5 + (by >> 1) * 4 + (bx >> 1)])
                        o = parent & 0xFFFFF if parent >> 20 & 1 else 0
                    gather(3, o, int(me_d[n, 21 + b]) & U32)
            for k in range(16):
                if x0 + (k & 3) * 16 + 16 <= w and y0 + (k >> 2) * 16 + 16 <= h:
                    gather(2, ois_dist(n, 5 + k), int(me_d[n, 5 + k]) & U32)
            for k in range(4):
                if x0 + (k & 1) * 32 + 32 <= w and y0 + (k >> 1) * 32 + 32 <= h:
                    gather(1, ois_dist(n, 1 + k), int(me_d[n, 1 + k]) & U32)
            if complete[n]:
                gather(0, ois_64(n) & U32, int(me_d[n, 0]) & U32)
        i_avg, e_avg = [0] * 4, [0] * 4
        for d in range(3 if jb["skip"] else 4):
            if not leaves[d]:                                            # no unit of this depth in the picture: the reference divides by 0
                continue
            i_avg[d], e_avg[d] = i_acc[d] // leaves[d], e_acc[d] // leaves[d]
            lo, hi = abs(_s32(i_min[d]) - _s32(i_avg[d])), _s32(i_max[d]) - _s32(i_avg[d])
            if lo < hi:
                i_max[d] = (i_avg[d] + lo) & U32
            else:
                i_min[d] = (i_avg[d] - hi) & U32
            lo = hi = 0
            if slice_type != 0:
                lo, hi = abs(_s32(e_min[d]) - _s32(e_avg[d])), _s32(e_max[d]) - _s32(e_avg[d])
            if lo < hi:
                e_max[d] = (e_avg[d] + lo) & U32
            else:
                e_min[d] = (e_avg[d] - hi) & U32
        for name, v in zip(("intra_complexity_min", "intra_complexity_max", "intra_complexity_accum", "intra_complexity_avg", "inter_complexity_min",
                            "inter_complexity_max", "inter_complexity_accum", "inter_complexity_avg", "processed_leaf_count"),
                           (i_min, i_max, i_acc, i_avg, e_min, e_max, e_acc, e_avg, leaves)):
            pic[name] = v
    return lcu, pic, parents
