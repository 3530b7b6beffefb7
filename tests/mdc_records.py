"""Seeded input records of the mode-decision configuration (ModeDecisionConfigurationKernel, Codec/EbModeDecisionConfigurationProcess.c:1905) in the form a
batched device entry behind svt_amd_source_ops_batch_launch would take them: what the stages in front of it leave per picture - ME records, 64x64 block statistics, detector records, the source-based operations' LCU and picture
records, the logo and noise flags - and the scalars the reference's host stages own, drawn around the thresholds the stage tests.  Shared by the fixture
generator (tests/golden/make_mdc_golden.py) and the CPU suite: the fixtures hold the case names and the reference's results only (with the
lambda and the two split-flag rates the reference's own tables gave each picture), the inputs are drawn again from the seed."""
import numpy as np

import svtlib as S
from pa_detect_numpy import LCU_DETECT_DTYPE
from sbo_records import SBO_LCU_DTYPE, SBO_PIC_DTYPE

PIC_DETECT_DTYPE = np.dtype([("pic_avg_variance", "<u2"), ("very_low_var_pic", "u1"), ("logo_pic", "u1"), ("lcu_block_percentage", "u1"), ("pad", "u1", 3)])
NOISE_PIC_DTYPE = np.dtype([("noise_variance_sum", "<u8"), ("block_count", "<u4"), ("pic_noise_class", "u1"), ("pad", "u1", 3)])
# the records the stage leaves: per LCU the leaf list in the order and widths of SvtAmdMdLcu (svtlib.MD_LCU_DTYPE), then the search method and what led to it;
# per picture the signals and the budgeting state
MDC_LCU_DTYPE = np.dtype([("leaf_count", "u1"), ("leaf_index", "u1", 85), ("leaf_split", "u1", 85), ("lcu_md_mode", "u1"), ("aura_status", "u1"), ("pred64", "u1"),
                          ("avc_partitioning", "u1"), ("pad0", "u1"), ("lcu_score", "<u4"), ("lcu_cost", "u1"), ("pad", "u1", 3)])
MDC_PIC_DTYPE = np.dtype([("scene_characteristic_id", "u1"), ("adjust_min_qp", "u1"), ("high_intra_selection", "u1"), ("slice_cb_qp_offset", "i1"),
                          ("slice_cr_qp_offset", "i1"), ("tc_offset", "i1"), ("beta_offset", "i1"), ("average_qp", "u1"),
                          ("adp_depth_sensitive_picture_class", "u1"), ("adp_refinement_mode", "u1"), ("number_of_segments", "u1"), ("pad0", "u1"),
                          ("budget", "<u4"), ("predicted_cost", "<u4"), ("lcu_min_score", "<u4"), ("lcu_max_score", "<u4"), ("score_th", "i1", 7),
                          ("interval_cost", "u1", 7), ("iterations", "u1"), ("bdp_present", "u1"), ("md_present", "u1"), ("pad", "u1", 3)])
assert PIC_DETECT_DTYPE.itemsize == 8 and NOISE_PIC_DTYPE.itemsize == 16 and MDC_LCU_DTYPE.itemsize == 184 and MDC_PIC_DTYPE.itemsize == 48
LCU_FIELDS = tuple(f for f in MDC_LCU_DTYPE.names if not f.startswith("pad"))
PIC_FIELDS = tuple(f for f in MDC_PIC_DTYPE.names if not f.startswith("pad"))
# EB_PICTURE_DEPTH_MODE / EB_LCU_DEPTH_MODE (Codec/EbDefinitions.h:1262-1280)
PICT_LCU_SWITCH, PICT_FULL85, PICT_FULL84, PICT_BDP, PICT_LIGHT_BDP, PICT_OPEN_LOOP = range(6)
LCU_FULL85, LCU_FULL84, LCU_BDP, LCU_LIGHT_BDP, LCU_OPEN_LOOP, LCU_LIGHT_OPEN_LOOP, LCU_AVC, LCU_LIGHT_AVC, LCU_PRED_OPEN_LOOP, LCU_PRED_OPEN_LOOP_1_NFL = range(1, 11)
INVALID_AURA_STATUS = 128


P, B = 1, 2
SCALARS = ("slice_type", "layer", "hier", "ref", "depth_mode", "enc_mode", "cls", "qp", "pan", "tilt", "ndth", "homog", "fr30", "cu8", "avg_int",
           "ref_int0", "ref_int1", "ref_intra0", "ref_intra1", "ref_layer0", "ref_layer1", "ref_skip0", "ref_skip1")


def job(slice_type, layer, ref, enc_mode, cls=0, qp=30, hier=3, depth_mode=PICT_LCU_SWITCH, noise=1, pan=0, tilt=0, ndth=0, homog=20, fr30=0, cu8=0, avg_int=100,
        ref_int=(100, 100), ref_intra=(0, 0), ref_layer=(0, 0), ref_skip=(0, 0), stationary="none", logo=0, dark=0, black=10, grass=0, nm_avg=20, zz_avg=20,
        intra_prob=10, spread="wide", bounds="inside", sharp=0.3):
    """the scalars of a job and the knobs of make_inputs.  stationary: 'none' (NULL pointer), 'some' or 'all'; spread: how the 64x64 distortions lie ('wide',
    'low_outlier', 'high_outlier', 'bulk'); bounds: where inter_complexity_min / max lie against them ('inside': some scores beyond both, 'outside')"""
    return dict(slice_type=slice_type, layer=layer, hier=hier, ref=ref, depth_mode=depth_mode, enc_mode=enc_mode, cls=cls, qp=qp, pan=pan, tilt=tilt, ndth=ndth,
                homog=homog, fr30=fr30, cu8=cu8, avg_int=avg_int, ref_int0=ref_int[0], ref_int1=ref_int[1], ref_intra0=ref_intra[0], ref_intra1=ref_intra[1],
                ref_layer0=ref_layer[0], ref_layer1=ref_layer[1], ref_skip0=ref_skip[0], ref_skip1=ref_skip[1], noise=noise, stationary=stationary, logo=logo,
                dark=dark, black=black, grass=grass, nm_avg=nm_avg, zz_avg=zz_avg, intra_prob=intra_prob, spread=spread, bounds=bounds, sharp=sharp)


def _usual_jobs(cls=0):
    """P and B pictures, layers 0..3, referenced and not, the six enc_mode rungs of SetTargetBudgetOq, QP 20 / 38 / 39 / 51, noise classes through 7, pan and tilt,
    stationary-edge bytes set and NULL, cu8x8_mode both ways, and one PICT_FULL85, PICT_FULL84 and PICT_BDP picture"""
    return [job(P, 0, 1, 3, cls, qp=20, noise=1, spread="low_outlier"),
            job(B, 0, 1, 5, cls, qp=38, noise=3, nm_avg=20, stationary="some", grass=20, zz_avg=16, spread="high_outlier"),
            job(B, 1, 1, 7, cls, qp=39, noise=4, dark=1, black=26, grass=61, ref_skip=(0, 0), fr30=1, nm_avg=26),
            job(B, 2, 0, 8, cls, qp=51, noise=5, pan=1, grass=40, cu8=1, logo=1, spread="bulk"),
            job(B, 3, 0, 9, cls, qp=30, noise=7, tilt=1, stationary="some", ref_skip=(1, 0), nm_avg=255),
            job(B, 1, 1, 11, cls, qp=38, noise=2, avg_int=100, ref_int=(100, 104), grass=70, hier=4, bounds="outside"),
            job(P, 0, 1, 9, cls, qp=39, noise=3, nm_avg=15, ref_int=(100, 100), cu8=1, spread="high_outlier"),
            job(B, 2, 1, 5, cls, qp=30, noise=1, dark=1, grass=61, intra_prob=60, stationary="some", fr30=1),
            job(B, 0, 1, 8, cls, qp=30, noise=6, ndth=1, grass=3, zz_avg=16, homog=49, intra_prob=60, ref_intra=(60, 60), spread="low_outlier"),
            job(B, 1, 0, 3, cls, qp=30, depth_mode=PICT_FULL85, stationary="some"),
            job(B, 2, 0, 7, cls, qp=39, depth_mode=PICT_FULL84),
            job(P, 0, 1, 3, cls, qp=30, depth_mode=PICT_BDP, noise=4)]


#          width, height, seed, jobs
CASES = {
    "one_64x64": (64, 64, 3, _usual_jobs()),                    # one LCU: min = max, subInterval 0, no aura candidate
    "aura_192x192": (192, 192, 5, _usual_jobs(cls=2)),          # exactly one LCU that can be judged for aura
    "whole_256x128": (256, 128, 7, _usual_jobs(cls=3)),         # whole LCUs: the last column and row count as inside (isEdgeLcu)
    "partial_416x240": (416, 240, 9, _usual_jobs()),            # partial right column and bottom row
    "many_704x640": (704, 640, 11, _usual_jobs(cls=2)),         # 110 LCUs: the 2 % bins and the percentage thresholds bite
    # class 3 forced on a small picture; every LCU carries a stationary edge in the first job, so the AVC refinement meets its budget in one pass
    "class3_704x640": (704, 640, 13, [job(B, 1, 1, 5, 2, stationary="all"), job(B, 0, 1, 8, 3, noise=4, nm_avg=20, dark=1, black=26),
                                      job(B, 1, 1, 9, 3, noise=3, nm_avg=16, black=30, fr30=1), job(B, 2, 0, 11, 3, noise=1, nm_avg=29, logo=1),
                                      job(P, 0, 1, 8, 3, noise=3, nm_avg=15), job(B, 3, 0, 3, 3, qp=39, stationary="some", dark=1, sharp=0.8)]),
}


def md_scan():
    """the 85 coded units in mode-decision order (GetCodedUnitStats, Codec/EbUtility.c): depth, size, origin and the raster-scan index of the ME records"""
    units = []

    def walk(depth, x, y):
        size = 64 >> depth
        units.append((depth, size, x, y, (0, 1, 5, 21)[depth] + (y // size) * (64 // size) + x // size))
        if depth < 3:
            for q in range(4):
                walk(depth + 1, x + (q & 1) * (size // 2), y + (q >> 1) * (size // 2))
    walk(0, 0, 0)
    return units


MD_SCAN = md_scan()
MD_TO_RASTER = np.array([u[4] for u in MD_SCAN])
assert MD_TO_RASTER[:8].tolist() == [0, 1, 5, 21, 22, 29, 30, 6] and MD_TO_RASTER[22] == 2


def geometry(w, h):
    wl, hl = (w + 63) // 64, (h + 63) // 64
    col, row = np.arange(wl * hl) % wl, np.arange(wl * hl) // wl
    complete = (col * 64 + 64 <= w) & (row * 64 + 64 <= h)
    edge = (col * 64 < 64) | (row * 64 < 64) | (col * 64 > w - 64) | (row * 64 > h - 64)     # isEdgeLcu (Codec/EbSequenceControlSet.c:210)
    return wl, hl, col, row, complete, edge


def unit_validity(w, h):
    """rasterScanCuValidity of every LCU in MD-scan order: [lcus][85]"""
    wl, hl, col, row, complete, edge = geometry(w, h)
    valid = np.zeros((wl * hl, 85), bool)
    for k, (depth, size, x, y, raster) in enumerate(MD_SCAN):
        valid[:, k] = (col * 64 + x + size <= w) & (row * 64 + y + size <= h)
    return valid


def make_inputs(w, h, seed, index, jb):
    """the records of job `index` of a case -> dict of arrays (stationary_edge: [lcus] bytes or None)"""
    rng = np.random.default_rng([seed, index, 18])
    wl, hl, col, row, complete, edge = geometry(w, h)
    n = wl * hl
    pick = lambda values, size: np.array(values)[rng.integers(0, len(values), size)]  # noqa: E731
    # ---- ME records: the 64x64 distortions by the kind of spread, the smaller units around a quarter of their parent ----
    spread = jb["spread"]
    d64 = rng.integers(5000, 60000, n)
    if spread == "bulk":                      # nine LCUs in ten lie in one tenth of the range
        d64 = np.where(rng.random(n) < 0.9, rng.integers(20000, 23000, n), d64)
    if spread == "low_outlier" and n > 60:
        d64 = rng.integers(30000, 60000, n)
        d64[rng.integers(0, n)] = 300
    if spread == "high_outlier" and n > 60:
        d64 = rng.integers(5000, 30000, n)
        d64[rng.integers(0, n)] = 300000
    if spread in ("wide", "bulk"):            # around AuraDetection64x64's 64 * 64
        near = rng.random(n) < 0.1
        d64[near] = pick((1000, 4096, 4097), int(near.sum()))
    me = np.zeros(n, S.ME_LCU_DTYPE)
    d32 = (d64[:, None] / 4 * rng.uniform(0.6, 1.4, (n, 4))).astype(np.int64)
    d16 = (d32[:, [(k >> 3) * 2 + ((k & 3) >> 1) for k in range(16)]] / 4 * rng.uniform(0.6, 1.4, (n, 16))).astype(np.int64)
    d8 = rng.integers(0, 2500, (n, 64))
    me["pu"]["distortion"][:, :, 0] = np.concatenate([d64[:, None], d32, d16, d8], 1)
    me["pu"]["distortion"][:, :, 1:] = rng.integers(0, 1 << 20, (n, 85, 2))
    mv = rng.integers(-12, 13, (n, 85, 4))
    far = rng.random((n, 85)) < 0.15
    mv[far] = rng.integers(-700, 701, (int(far.sum()), 4))
    still = rng.random(n) < 0.3               # LCUs whose 64x64 vectors stay below every GLOBAL_MOTION_THRESHOLD
    mv[still, 0] = rng.integers(-2, 3, (int(still.sum()), 4))
    me["pu"]["mv"] = mv
    if jb["slice_type"] == B:
        order = np.argsort(rng.random((n, 85, 3)), 2)
        me["pu"]["direction"] = order
        me["pu"]["total"] = pick((1, 2, 3, 3), (n, 85))
    else:
        me["pu"]["direction"], me["pu"]["total"] = 0, 1
    # ---- block statistics and detector records: what the stage reads, the rest anything ----
    stats = np.zeros(n, S.PA_LCU_STATS_DTYPE)
    stats["variance"] = rng.integers(0, 2000, (n, 85))
    stats["y_mean"] = rng.integers(0, 256, (n, 85))
    stats["variance"][:, 0] = pick((50, 100, 101, 400), n)
    stats["y_mean"][:, 0] = pick((10, 24, 25, 100, 200), n)
    detect = np.zeros(n, LCU_DETECT_DTYPE)
    interior = (col > 0) & (col < wl - 1) & (row > 0) & (row < hl - 1)
    detect["edge_block_num"] = (interior | (n < 4)) & (rng.random(n) < 0.4)
    detect["sharp_edge"] = rng.random(n) < jb["sharp"]
    detect["homogeneous"] = rng.random(n) < 0.5
    detect["edge_cu"] = rng.integers(0, 65536, n)
    # ---- the source-based operations' records ----
    sbo_lcu = np.zeros(n, SBO_LCU_DTYPE)
    sbo_lcu["similar_colocated_all_layers"] = rng.random(n) < 0.5
    sbo_lcu["similar_colocated"] = sbo_lcu["similar_colocated_all_layers"] & jb["ref"]
    sbo_lcu["failing_motion"] = complete & (rng.random(n) < 0.1)
    sbo_lcu["non_moving_index"] = pick((0, 9, 10, 20, 25, 30, 30, 255), n)
    sbo_lcu["zz_cost"] = rng.integers(0, 31, n)
    sbo_lcu["complex_lcu"] = np.where(rng.random(n) < 0.06, 2, rng.integers(0, 2, n))
    sbo_lcu["grass"] = rng.integers(0, 65536, n)
    sbo_pic = np.zeros(1, SBO_PIC_DTYPE)
    p = sbo_pic[0]
    p["complete_lcu_count"], p["zz_cost_average"], p["non_moving_index_average"] = int(complete.sum()), jb["zz_avg"], jb["nm_avg"]
    p["grass_percentage"], p["high_dark_low_light_area_density"], p["black_area_percentage"] = jb["grass"], jb["dark"], jb["black"]
    p["intra_coded_block_probability"] = jb["intra_prob"]
    lo, hi = int(d64.min()), int(d64.max())
    if jb["bounds"] == "inside":              # as the trimmed bounds of the QPM statistics lie: some distortions below the minimum and above the maximum
        p["inter_complexity_min"][0], p["inter_complexity_max"][0] = lo + (hi - lo) // 8, hi - (hi - lo) // 8
    else:
        p["inter_complexity_min"][0], p["inter_complexity_max"][0] = lo // 2, hi + 1000
    p["inter_complexity_min"][1:], p["inter_complexity_max"][1:] = rng.integers(0, 1000, 3), rng.integers(1000, 9000, 3)
    p["inter_complexity_avg"] = rng.integers(0, 9000, 4)
    pic_detect = np.zeros(1, PIC_DETECT_DTYPE)
    pic_detect["logo_pic"], pic_detect["pic_avg_variance"] = jb["logo"], rng.integers(0, 3000)
    noise_pic = np.zeros(1, NOISE_PIC_DTYPE)
    noise_pic["pic_noise_class"], noise_pic["block_count"] = jb["noise"], n
    stationary = None
    if jb["stationary"] != "none":
        stationary = (np.ones(n, np.uint8) if jb["stationary"] == "all" else (rng.random(n) < 0.15).astype(np.uint8) * pick((1, 2), n).astype(np.uint8))
    return dict(me=me, stats=stats, detect=detect, sbo_lcu=sbo_lcu, sbo_pic=sbo_pic, pic_detect=pic_detect, noise_pic=noise_pic, stationary_edge=stationary)


def case_inputs(name):
    w, h, seed, jobs = CASES[name]
    return [make_inputs(w, h, seed, i, jb) for i, jb in enumerate(jobs)]
