"""Seeded input records of the batched source-based operations (include/svt_hevc_amd.h "Batched source-based operations"): what the stages in front of
SourceBasedOperationsKernel leave per picture - block statistics, chroma means, detector records, luma histograms, the zz records of the look-ahead window,
ME and OIS records - drawn around every threshold the stage tests, so that each is met from both sides.  Shared by the fixture generator
(tests/golden/make_sbo_golden.py), the CPU suite and the GPU suite: the fixtures hold the case names and the reference's results only, the inputs are drawn
again from the seed."""
import ctypes as C

import numpy as np

import svtlib as S
from pa_detect_numpy import LCU_CHROMA_DTYPE, LCU_DETECT_DTYPE
from sidelib import ZZ_DTYPE

SBO_LCU_DTYPE = np.dtype([("grass", "<u2"), ("skin", "<u2"), ("high_luma", "<u2"), ("high_chroma", "<u2"), ("zz_cost", "u1"), ("non_moving_index", "u1"),
                          ("similar_colocated", "u1"), ("similar_colocated_all_layers", "u1"), ("failing_motion", "u1"), ("uncovered_area", "u1"),
                          ("cmplx_contrast", "u1"), ("isolated_non_homogeneous", "u1"), ("cmplx_status", "u1"), ("complex_lcu", "u1"), ("pad", "u1", 6)])
QPM_FIELDS = ("intra_complexity_min", "intra_complexity_max", "intra_complexity_accum", "intra_complexity_avg", "inter_complexity_min", "inter_complexity_max",
              "inter_complexity_accum", "inter_complexity_avg", "processed_leaf_count")
SBO_PIC_DTYPE = np.dtype([("complete_lcu_count", "<u4"), ("zz_cost_average", "<u4"), ("non_moving_index_average", "<u2"), ("low_motion_content", "u1"),
                          ("dark_background_light_foreground", "u1"), ("intra_coded_block_probability", "u1"), ("grass_percentage", "u1"),
                          ("percentage_of_edge_in_light_background", "u1"), ("high_dark_area_density", "u1"), ("high_dark_low_light_area_density", "u1"),
                          ("black_area_percentage", "u1"), ("pad", "u1", 6)] + [(f, "<u4", 4) for f in QPM_FIELDS])
assert SBO_LCU_DTYPE.itemsize == 24 and SBO_PIC_DTYPE.itemsize == 168
LCU_FIELDS = tuple(f for f in SBO_LCU_DTYPE.names if f != "pad")
PIC_FIELDS = tuple(f for f in SBO_PIC_DTYPE.names if f != "pad")
SBO_LCU, SBO_PICTURE = 0, 1
ENTRY = "svt_amd_source_ops_batch_launch"
MAX_WINDOW = 17


class SboJob(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("ref_stats", C.c_void_p), ("chroma", C.c_void_p), ("detect", C.c_void_p), ("histogram", C.c_void_p),
                ("zz", C.c_void_p * MAX_WINDOW), ("me", C.c_void_p), ("ois", C.c_void_p), ("cur_slot", C.c_int32), ("zz_count", C.c_uint8),
                ("slice_type", C.c_uint8), ("temporal_layer_index", C.c_uint8), ("is_used_as_reference", C.c_uint8), ("resolution_class", C.c_uint8),
                ("skip_ois_8x8", C.c_uint8), ("cu8x8_mode", C.c_uint8), ("want_qpm", C.c_uint8), ("pad", C.c_uint8 * 4)]


class SboArrays(C.Structure):
    _fields_ = [("lcu", C.c_void_p), ("picture", C.c_void_p)]


def declare(lib):
    lib.svt_amd_source_ops_batch_launch.restype = C.c_int
    lib.svt_amd_source_ops_batch_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_void_p]
    lib.svt_amd_source_ops_bytes.restype, lib.svt_amd_source_ops_bytes.argtypes = C.c_size_t, [C.c_uint16, C.c_uint16, C.c_int]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib


I, P, B = 0, 1, 2


def job(slice_type, layer, ref, zz_count, skip=0, qpm=0, cu8=0, cls=0, activity="mixed", hist="bright", triggers=(), no_grass=0):
    return dict(no_grass=no_grass, slice_type=slice_type, layer=layer, ref=ref, zz_count=zz_count, skip=skip, qpm=qpm, cu8=cu8, cls=cls, activity=activity, hist=hist,
                triggers=tuple(triggers))


def _usual_jobs(cls=0, triggers=()):
    """I, P and B pictures; layers 0, 1, 2; referenced and not; windows of 0, 1 and 17 pictures; skip_ois_8x8 both ways; every activity and histogram kind"""
    return [job(I, 0, 1, 0, qpm=1, cls=cls, hist="dark"),
            job(I, 0, 1, 17, skip=1, qpm=1, cls=cls, activity="still", hist="dark_light"),
            job(P, 0, 1, 1, cls=cls, hist="wrap"),
            job(P, 0, 1, 17, qpm=1, cls=cls, activity="active"),
            job(B, 0, 1, 17, cls=cls, activity="moderate", triggers=triggers, hist="dark"),
            job(B, 1, 1, 17, skip=1, qpm=1, cls=cls, activity="active", triggers=triggers),
            job(B, 1, 0, 1, qpm=1, cu8=1, cls=cls, activity="moderate", triggers=triggers, hist="dark_light"),
            job(B, 2, 0, 17, cls=cls, triggers=triggers),
            job(B, 2, 1, 0, cls=cls, triggers=triggers)]


#          width, height, regions_w, regions_h, seed, jobs
CASES = {
    "one_64x64": (64, 64, 1, 1, 3, _usual_jobs()),                       # one LCU: no interior, no neighbour
    "interior_192x192": (192, 192, 2, 2, 5, _usual_jobs()),              # exactly one interior LCU
    "plain_320x256": (320, 256, 4, 4, 7, _usual_jobs()),
    "partial_416x240": (416, 240, 4, 4, 9, _usual_jobs(triggers=(5, 6, 12, 13, 18))),   # partial right column and bottom row; triggers next to both
    # 11 x 10 LCUs: contrast triggers at adjacent LCUs, horizontally (36, 37), vertically (62, 73) and on both diagonals (80, 92 / 26, 36)
    "pairs_704x640": (704, 640, 4, 4, 11, _usual_jobs(triggers=(26, 36, 37, 62, 73, 80, 92))),
    "class3_256x192": (256, 192, 2, 2, 13, [job(B, 1, 1, 17, qpm=1, cls=3, activity="active"), job(B, 0, 1, 17, cls=3, activity="active"),
                                            job(B, 2, 0, 17, cls=3, activity="moderate", hist="dark_no_white"), job(P, 0, 1, 2, cls=3, activity="active")]),
    # two pictures on ONE uncleared object: the second has no grass / skin where the first had some
    "sticky_192x128": (192, 128, 2, 2, 17, [job(I, 0, 1, 1, activity="mixed"), job(B, 1, 0, 1, activity="mixed", hist="dark", no_grass=1)]),
}

Y_VALUES = (40, 52, 53, 60, 70, 71, 100, 129, 130, 144, 145, 150, 180, 181, 200)
CB_VALUES = (80, 81, 100, 101, 105, 114, 115, 119, 120, 130, 131, 140, 149, 150, 151)
CR_VALUES = (79, 80, 100, 101, 110, 111, 115, 120, 126, 127, 129, 130, 134, 135, 136, 140, 159, 160)
VAR16_VALUES = (5, 10, 11, 100, 299, 300, 500)
VAR64_VALUES = (0, 30, 50, 51, 100, 101, 150, 400)
MEAN64_VALUES = (20, 44, 45, 100, 149, 150, 200)
ME32_VALUES = (1000, 5119, 5120, 10239, 10240, 26624, 27647, 27648, 28672, 29696, 33792, 34815, 34816, 60000)
FACTORS = (0.5, 0.9, 1.0, 1.14, 1.15, 1.16, 1.17, 1.2, 1.21, 1.22, 1.3, 2.0)
#          y, cb, cr of a 16x16 unit
THEMES = {1: (100, 105, 120),   # grass
          2: (100, 110, 140),   # skin
          3: (100, 140, 115),   # SpatialHighContrastClassifier
          4: (200, 152, 130)}   # high luma, high chroma


def geometry(w, h):
    wl, hl = (w + 63) // 64, (h + 63) // 64
    col, row = np.arange(wl * hl) % wl, np.arange(wl * hl) // wl
    complete = (col * 64 + 64 <= w) & (row * 64 + 64 <= h)
    return wl, hl, col, row, complete


def make_inputs(w, h, rw, rh, seed, index, jb):
    """the records of job `index` of a case -> dict of arrays (zz: [zz_count][lcus])"""
    rng = np.random.default_rng([seed, index])
    wl, hl, col, row, complete = geometry(w, h)
    n = wl * hl
    pick = lambda values, size: np.array(values)[rng.integers(0, len(values), size)]  # noqa: E731
    theme = rng.integers(0, 5, n)
    if jb["no_grass"]:
        theme[:] = 0
    theme[list(jb["triggers"])] = 3
    stats = np.zeros(n, S.PA_LCU_STATS_DTYPE)
    chroma = np.zeros(n, LCU_CHROMA_DTYPE)
    stats["variance"] = rng.integers(0, 2000, (n, 85))
    stats["y_mean"] = rng.integers(0, 256, (n, 85))
    stats["variance"][:, 5:21] = pick(VAR16_VALUES, (n, 16))
    stats["y_mean"][:, 5:21] = pick(Y_VALUES, (n, 16))
    chroma["cb_mean"] = pick(CB_VALUES, (n, 21))
    chroma["cr_mean"] = pick(CR_VALUES, (n, 21))
    for t, (y, cb, cr) in THEMES.items():
        on = (theme == t)[:, None] & (rng.random((n, 16)) < 0.7)
        if t == 3:
            on[list(jb["triggers"])] = True
        stats["y_mean"][:, 5:21][on], chroma["cb_mean"][:, 5:21][on], chroma["cr_mean"][:, 5:21][on] = y, cb, cr
        if t == 3:
            stats["variance"][:, 5:21][on] = 100
    if jb["no_grass"]:                        # neither grass nor skin in any unit
        chroma["cb_mean"][:, 5:21] = 150
    # the 64x64 variance: a busy left part and a flat right part, a quarter of the LCUs anything
    v64 = np.where(col <= wl // 2, 150, 40)
    anything = rng.random(n) < 0.25
    v64[anything] = pick(VAR64_VALUES, int(anything.sum()))
    stats["variance"][:, 0] = v64
    stats["y_mean"][:, 0] = pick(MEAN64_VALUES, n)
    # the reference picture: the same 64x64 values moved by steps around the two thresholds of 10
    ref_stats = stats.copy()
    ref_stats["y_mean"][:, 0] = np.clip(stats["y_mean"][:, 0].astype(int) + pick((0, 5, 9, -9, 10, -10, 20), n), 0, 255)
    cur = stats["variance"][:, 0].astype(np.int64)
    how = rng.integers(0, 7, n)
    ref_var = np.select([how == 0, how == 1, how == 2, how == 3, how == 4, how == 5], [cur, cur + 9, cur + 10, cur * 100 // 105, cur * 100 // 125, 0], 1)
    ref_stats["variance"][:, 0] = np.clip(ref_var, 0, 65535)
    # detector records: edge_block_num only where the detectors can set it (LCUs with a neighbour on every side)
    detect = np.zeros(n, LCU_DETECT_DTYPE)
    detect["var_of_var_32x32"] = pick((0, 4096, 4097, 1000000), (n, 4)).astype(np.uint64)
    detect["var_of_var_32x32"][~complete] = np.uint64(0xFFFFFFFFFFFFFFFF)
    detect["homogeneous"] = rng.random(n) < 0.6
    interior = (col > 0) & (col < wl - 1) & (row > 0) & (row < hl - 1)
    detect["edge_block_num"] = interior & (rng.random(n) < 0.5)
    stats["y_mean"][:, 0][interior & (rng.random(n) < 0.5)] = 150
    detect["edge_cu"] = rng.integers(0, 65536, n)
    # luma histograms: bins that start at 1 and end << 4, the picture's samples spread by the kind
    area = w * h
    dark, mid = dict(bright=(0.05, 0.03), wrap=(0.05, 0.03), dark=(0.3, 0.02), dark_no_white=(0.3, 0.02), dark_light=(0.17, 0.12))[jb["hist"]]
    weights = np.empty(256)                   # the share of the samples below 25, in 25..39 and above
    weights[:25], weights[25:40], weights[40:] = dark / 25, mid / 15, (1 - dark - mid) / 216
    total = np.floor(weights * area / (rw * rh))
    histogram = np.zeros((rw, rh, 256), np.uint32)
    histogram[:] = ((total.astype(np.uint32) >> 4) + 1) << 4
    histogram[0, 0, rng.integers(0, 256, 8)] += 16
    if jb["hist"] == "dark_no_white":
        histogram[:, :, 210:] = 0
    if jb["hist"] == "wrap":                  # counts whose product with 100 leaves 32 bits (:703, :721)
        histogram[0, 0, 3], histogram[rw - 1, rh - 1, 30], histogram[0, rh - 1, 250] = 50000000, 43000000, 42949673
    # the look-ahead window
    zz = np.zeros((jb["zz_count"], n), ZZ_DTYPE)
    if jb["zz_count"]:
        act = jb["activity"]
        base_nm = np.where(col <= wl // 2, 30, 0) if act == "mixed" else np.full(n, dict(active=30, moderate=30, still=0)[act])
        if act == "moderate":                 # a fifth of the LCUs rests: the average lands between 23 and 29
            base_nm[rng.permutation(n)[:max(1, n // 5)]] = 0 if n > 4 else 10
        base_zz = np.where(base_nm == 30, 30, 0)
        for k in range(jb["zz_count"]):
            nm, zc = base_nm.copy(), base_zz.copy()
            flicker = rng.random(n) < dict(still=0.0, active=0.005, moderate=0.01, mixed=0.15)[act]
            nm[flicker], zc[flicker] = pick((0, 10, 20, 30), int(flicker.sum())), pick((0, 3, 10, 20, 30), int(flicker.sum()))
            zz[k]["non_moving_index"], zz[k]["zz_cost"] = nm, zc
            zz[k]["sad"] = np.where(complete, rng.integers(0, 1 << 20, n), 0xFFFFFFFF)
    # ME and OIS records: only what the stage reads is drawn (distortion[0] of every unit, candidate[unit][0]); the rest stays 0
    me, ois = np.zeros(n, S.ME_LCU_DTYPE), np.zeros(n, S.OIS_LCU_DTYPE)
    me32 = pick(ME32_VALUES, (n, 4)).astype(np.int64)
    quiet = theme != 3
    me32[quiet & (rng.random(n) < 0.5)] = 1000                                      # LCUs without high distortion
    me32[list(jb["triggers"])] = 40000
    ois32 = np.minimum((me32 / pick(FACTORS, (n, 4))).astype(np.int64), 0xFFFFF)
    ois32[rng.random((n, 4)) < 0.05] = 0
    ois64 = ois32.sum(1)
    me64 = (ois64 * pick(FACTORS, n)).astype(np.int64)
    huge = rng.random(n) < 0.05
    if not jb["qpm"]:                         # (EB_S32) of it is negative (:211); kept out of the QPM bounds, whose signed differences it would overflow
        me64[huge] = 0xFFFFFF00
    me16 = rng.integers(0, 20000, (n, 16))
    me8 = rng.integers(0, 6000, (n, 64))
    dist = np.concatenate([me64[:, None], me32, me16, me8], 1)
    me["pu"]["distortion"][:, :, 0] = dist
    me["pu"]["distortion"][:, :, 1:] = rng.integers(0, 1 << 20, (n, 85, 2))
    o_dist = np.concatenate([np.zeros((n, 1), np.int64), ois32, rng.integers(0, 30000, (n, 16)), rng.integers(0, 8000, (n, 64))], 1)
    valid = rng.random((n, 85)) < 0.7
    word = o_dist.astype(np.uint32) | (valid.astype(np.uint32) << 20) | (rng.integers(0, 8, (n, 85)).astype(np.uint32) << 21) | \
        (rng.integers(0, 35, (n, 85)).astype(np.uint32) << 24)
    ois["candidate"][:, :, 0] = word
    ois["candidate"][:, :, 1:] = rng.integers(0, 1 << 32, (n, 85, 17), dtype=np.uint64).astype(np.uint32)
    ois["total"] = rng.integers(1, 18, (n, 85))
    return dict(stats=stats, ref_stats=ref_stats, chroma=chroma, detect=detect, histogram=histogram, zz=zz, me=me, ois=ois)


def case_inputs(name):
    w, h, rw, rh, seed, jobs = CASES[name]
    return [make_inputs(w, h, rw, rh, seed, i, jb) for i, jb in enumerate(jobs)]
