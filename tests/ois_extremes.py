"""Builders for the open-loop intra search at the ends of its range, shared by tests/test_ois_extremes_cpu.py and tests/test_gpu_ois_extremes.py.
numpy and the CPU oracle only: no product library, no GPU.

A 32x32 CU is SATURATED when every one of its 35 predictions misses every sample by 255: the oracle's ois_kernel_level = 1 run of the picture ranks its
best distortion at 32 * 32 * 255 = 261,120.  On the stage-1 path no mode of such a CU beats the reference's initial best, so it is CARRIED when it tests
any mode at all (total > 1): its candidate list comes from the best mode of the CU before it in the LCU, its first distortion out of the array the CUs
before it wrote (mode 30 and distortion 0 when none did)."""
import ctypes as C

import numpy as np

import svtlib as S

SAT = 32 * 32 * 255  # 261,120
ISLANDS = ("x_islands", 320, 256, 3)  # kind, width, height, seed
# the ME SADs of the seeded island jobs: around every threshold of the three sets once divided by a DC SAD of 261,120 ((me - dc) * 100 / dc = -99, -20, -19,
# 0, 0, 150, 200, 200, 300); the largest, a 64x64 SAD, times 100 stays below 2^31
ME_VALUES = np.array([1, SAT * 4 // 5, SAT * 4 // 5 + 1, SAT, SAT + 1, SAT * 5 // 2, 3 * SAT, 3 * SAT + 1, 4 * SAT], np.uint32)
assert int(ME_VALUES.max()) == 1044480 and int(ME_VALUES.max()) * 100 < 2 ** 31


def params(w, h, **kw):
    p = S.OisParams()
    p.luma_width, p.luma_height = w, h
    p.ois_th_set = 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def me_of(sad):
    """ME_LCU_DTYPE records that carry only distortion[0], all the search reads of them"""
    me = np.zeros(len(sad), S.ME_LCU_DTYPE)
    me["pu"]["distortion"][:, :, 0] = sad
    return me


_frames, _sat = {}, {}


def frame(kind, w, h, t, seed):
    key = (kind, w, h, t, seed)
    if key not in _frames:
        f = S.gen_luma(kind, w, h, t, seed)
        f.setflags(write=False)
        _frames[key] = f
    return _frames[key]


def saturated(oracle, kind, w, h, t, seed):
    """bool [LCUs, 4]: the 32x32 CUs 1..4 whose best of 35 distortions is 261,120"""
    key = (kind, w, h, t, seed)
    if key not in _sat:
        r = S.oracle_ois_picture(oracle, params(w, h, ois_kernel_level=1, skip_ois_8x8=1), frame(*key), None)
        _sat[key] = ((r["candidate"][:, 1:5, 0] & 0xFFFFF) == SAT) & (r["total"][:, 1:5] == 18)
    return _sat[key]


def stage1_path(p):
    return not (p["slice_is_intra"] or p["ois_kernel_level"] or p["limit_ois_to_dc_mode"])


def carried(sat, record):
    """bool [LCUs, 4] of a stage-1 record (OIS_LCU_DTYPE array of the picture's LCUs)"""
    tot = record["total"][:, 1:5]
    return sat & (tot > 1) & (tot != 0xFF)


# ---- part 4b: seeded island jobs ----

ISLAND_JOBS = [dict(ois_th_set=s, temporal_layer_index=l, set_best_ois_distortion_to_valid=v, skip_ois_8x8=k, cu8x8_mode=k)
               for s in (0, 1, 2) for l in (0, 2, 3) for v in (0, 1) for k in (0, 1)]
_island_jobs = {}


def island_job(oracle, j):
    """Job j of ISLAND_JOBS: (frame, OisParams, ME records, the oracle's records).  Frames t = 1 (white ground) and t = 3 (black ground) in turn; in every
    other job the CUs 2 and 3 of the twin LCU get ME SAD 1, the value most likely to leave them at the DC mode alone, so that CU 4 follows CU 1 directly."""
    if j not in _island_jobs:
        kind, w, h, seed = ISLANDS
        t = 1 + 2 * (j & 1)
        luma = frame(kind, w, h, t, seed)
        rng = np.random.default_rng([41, j])
        sad = ME_VALUES[rng.integers(0, len(ME_VALUES), (S.lcu_count(w, h), 85))]
        if (j >> 1) & 1:
            for ox, oy in S.islands_layout(w, h, t, seed)["twins"]:
                sad[(oy // 64) * ((w + 63) // 64) + ox // 64, 2:4] = 1
        p = params(w, h, **ISLAND_JOBS[j])
        me = me_of(sad)
        want = S.oracle_ois_picture(oracle, p, luma, me)
        for a in (me, want):
            a.setflags(write=False)
        _island_jobs[j] = (luma, p, me, want, saturated(oracle, kind, w, h, t, seed))
    return _island_jobs[j]


# ---- plain restatement of the two N < 32 edge filters (H.265 8.4.4.2.5 / 8.4.4.2.6 with disableIntraBoundaryFilter = 0) ----

def neighbours(luma, ox, oy, n):
    """left[0 .. 2N-1] top-to-bottom, top-left, top[0 .. 2N-1]; 128 outside the picture or where the picture has no row above / column to the left"""
    h, w = luma.shape
    left, top, tl = [128] * (2 * n), [128] * (2 * n), 128
    if ox:
        for i in range(min(2 * n, h - oy)):
            left[i] = int(luma[oy + i, ox - 1])
    if ox and oy:
        tl = int(luma[oy - 1, ox - 1])
    if oy:
        for i in range(min(2 * n, w - ox)):
            top[i] = int(luma[oy - 1, ox + i])
    return left, tl, top


def edge_filter_extremes(luma, ox, oy, n):
    """Of the CU at (ox, oy), N < 32: (samples of the mode-26 / mode-10 edge filter below 0 before the clip, above 255, DC-filtered edge samples whose
    neighbour lies 127 or more below the DC value, above it: a CU with one edge at 0 and the other at 255 has DC value 128)"""
    left, tl, top = neighbours(luma, ox, oy, n)
    raw = [top[0] + ((left[i] - tl) >> 1) for i in range(n)] + [left[0] + ((top[i] - tl) >> 1) for i in range(n)]
    dc = (sum(left[:n]) + sum(top[:n]) + n) >> (n.bit_length())
    edge = left[:n] + top[:n]
    return (sum(v < 0 for v in raw), sum(v > 255 for v in raw), sum(v - dc <= -127 for v in edge), sum(v - dc >= 127 for v in edge))


# ---- ComputeDecimatedZzSad through the oracle (SvtAmdZzLcu records) ----

ZZ_DTYPE = np.dtype([("sad", "<u4"), ("zz_cost", "u1"), ("non_moving_index", "u1"), ("pad", "u1", 2)])


def oracle_zz(oracle, cur, prev):
    h, w = cur.shape
    out = np.zeros(S.lcu_count(w, h), ZZ_DTYPE)
    oracle.svt_oracle_zz_sad_picture.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    oracle.svt_oracle_zz_sad_picture.restype = None
    oracle.svt_oracle_zz_sad_picture(np.ascontiguousarray(cur).ctypes.data, np.ascontiguousarray(prev).ctypes.data, w, w, h, out.ctypes.data)
    return out
