"""Seeded input records of the initial rate control's look-ahead stage (InitialRateControlKernel, Codec/EbInitialRateControlProcess.c:849, with the checks in
front of it and the stationary-edge stage behind it) in the form the batched device entry svt_amd_initial_rc_batch_launch takes them: what the stages in front of
it leave per picture - the 64x64 unit's vector and distortion of the ME records, the block variances, the detector's edge_cu bits - for a SEQUENCE of pictures,
so that the look-ahead windows of neighbouring pictures overlap, and the queue state the reference's host owns: POCs, slice types, end-of-sequence and
scene-change flags, where the head stands.  Shared by the fixture generator (tests/golden/make_irc_golden.py), the CPU suite and the GPU suite: the fixtures hold
the case names and the reference's results only, the inputs are drawn again from the seed."""
import numpy as np

import svtlib as S
from pa_detect_numpy import LCU_DETECT_DTYPE

CHECKS_DTYPE = np.dtype([("check1", "u1"), ("pm_check1", "u1"), ("check2", "u1"), ("low_dist_logo", "u1")])
MOTION_DTYPE = np.dtype([("total_checked_lcus", "<u4"), ("total_pan_lcus", "<u4"), ("total_tilt_lcus", "<u4"), ("total_pan_high_amp_lcus", "<u4"),
                         ("total_tilt_high_amp_lcus", "<u4"), ("is_pan_raw", "u1"), ("is_tilt_raw", "u1"), ("pad", "u1", 2)])
IRC_LCU_DTYPE = np.dtype([("similar_edge_count", "u1", 16), ("pm_similar_edge_count", "u1", 16), ("var_of_var_over_time", "<u8"), ("homogeneous_over_time", "u1"),
                          ("motion_votes", "u1"), ("pad", "u1", 6)])
IRC_PIC_DTYPE = np.dtype([("is_pan", "u1"), ("is_tilt", "u1"), ("homogeneity_percentage", "u1"), ("pad0", "u1"), ("homogeneous_lcu_count", "<u2"),
                          ("stationary_lcu_count", "<u2", 4), ("pad", "u1", 2)])
assert CHECKS_DTYPE.itemsize == 4 and MOTION_DTYPE.itemsize == 24 and IRC_LCU_DTYPE.itemsize == 48 and IRC_PIC_DTYPE.itemsize == 16
CHECKS_FIELDS = CHECKS_DTYPE.names
MOTION_FIELDS = tuple(f for f in MOTION_DTYPE.names if not f.startswith("pad"))
LCU_FIELDS = tuple(f for f in IRC_LCU_DTYPE.names if not f.startswith("pad"))
PIC_FIELDS = tuple(f for f in IRC_PIC_DTYPE.names if not f.startswith("pad"))
QUEUE_DEPTH = 2048                      # INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH (Codec/EbEncodeContext.h:37)

I, P, B = 0, 1, 2
LAYER_OF_POC = (0, 3, 2, 3, 1, 3, 2, 3)   # a four-layer hierarchy: the layer of POC & 7


def pic(slice_type=B, layer=None, motion="pan", scene=0, hier=3):
    """one picture of a sequence: its POC is its place; layer None: LAYER_OF_POC.  motion: 'pan', 'tilt', 'still' or 'mixed' - how the 64x64 vectors lie"""
    return dict(slice_type=slice_type, layer=layer, motion=motion, scene=scene, hier=hier)


def sequence(pics, lad, period, head0, strong=(), medium=()):
    """a case's queue state.  Picture k has POC k, sits at queue index (head0 + k) % QUEUE_DEPTH and leaves the stage as the k-th; the last one carries the
    end-of-sequence flag.  lad: lookAheadDistance; period: predStructPeriod; strong / medium: (column, row) of the LCUs that hold a persistent logo block whose
    32x32 variances spread beyond check1's / pm_check1's threshold - every other LCU is flat; both empty: the kinds are drawn"""
    pics = [dict(p, poc=k, layer=LAYER_OF_POC[k & 7] if p["layer"] is None else p["layer"], eos=int(k == len(pics) - 1)) for k, p in enumerate(pics)]
    return dict(pics=pics, lad=lad, period=period, head0=head0, strong=tuple(strong), medium=tuple(medium))


def _run(n, motions, first=I, scene_at=(), intra_at=(), p_at=()):
    """n pictures: the first an I picture, motion by the pattern `motions` (one letter a picture, repeated: p pan, t tilt, s still, m mixed)"""
    names = dict(p="pan", t="tilt", s="still", m="mixed")
    out = []
    for k in range(n):
        st = first if k == 0 else I if k in intra_at else P if k in p_at else B
        out.append(pic(st, 0 if st == I else None, names[motions[k % len(motions)]], int(k in scene_at)))
    return out


def _usual_jobs():
    """a sequence for any geometry: I, P and B pictures of every layer, pan, tilt, still and mixed motion, a scene change and a second I picture inside the windows,
    frames_to_check falling from 9 to 1 at the sequence end, the head passing the last queue index; the kinds of the LCUs are drawn"""
    return sequence(_run(13, "pppppptsmppp", scene_at=(6,), intra_at=(9,), p_at=(4,)), lad=9, period=4, head0=QUEUE_DEPTH - 5)


#          width, height, resolution class, seed, sequence
CASES = {
    "one_64x64": (64, 64, 0, 3, sequence(_run(10, "ppppsptppp"), 8, 4, QUEUE_DEPTH - 8)),
    # the three logo regions of class 0 (3 x 2 LCUs in the top corners, the two bottom rows) around an interior that is none.  Bottom band: two pairs of strong blocks
    # four columns apart - the LCUs between them become 2 and 3 -, top left: a lone strong block (cleared), top right: a pair of medium blocks (the PM plane only)
    "corners_704x640": (704, 640, 0, 5, sequence(_run(20, "ppppppppttmsppppmmpt", p_at=(8,)), 17, 8, QUEUE_DEPTH - 4,
                                                 strong=((1, 8), (2, 8), (6, 8), (7, 8), (0, 0)), medium=((9, 0), (10, 0), (4, 9)))),
    "partial_416x240": (416, 240, 0, 7, sequence(_run(12, "pptsppmppppp"), 8, 4, 10, strong=((4, 2), (5, 2), (1, 0)), medium=((0, 2), (1, 2)))),
    "class1_1024x576": (1024, 576, 1, 9, sequence(_run(10, "ppppppptsm"), 8, 4, QUEUE_DEPTH - 2)),
    "class3_2112x1152": (2112, 1152, 3, 11, sequence(_run(10, "tttttttpsm", p_at=(4,)), 8, 4, 0)),
    # the sequence end: frames_to_check falls from 17 to 1, the threshold wraps below 4, the last picture has no look-ahead
    "tail_192x128": (192, 128, 0, 13, sequence(_run(20, "pppppppppppptttttmsp"), 17, 8, QUEUE_DEPTH - 3, strong=((0, 0), (1, 0), (1, 1)), medium=((2, 1),))),
    "scene_256x192": (256, 192, 0, 15, sequence(_run(14, "ppppptttpppmsp", scene_at=(5, 11), intra_at=(5, 9)), 12, 8, QUEUE_DEPTH - 6,
                                                strong=((0, 0), (1, 0), (3, 2)), medium=((2, 2), (1, 1)))),
    # a sequence that ENDS in an I picture: no look-ahead, an all-zero motion record, the reset homogeneity records, ME records that nobody reads
    "ends_intra_128x64": (128, 64, 0, 17, sequence(_run(4, "ppsp", intra_at=(3,)), 3, 1, QUEUE_DEPTH - 2, strong=((0, 0),), medium=((1, 0),))),
}


def geometry(w, h, cls):
    """-> wl, hl, col, row, isCompleteLcu, potentialLogoLcu (Codec/EbSequenceControlSet.c:206, :216-273: the comparisons are signed)"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    col, row = np.arange(wl * hl) % wl, np.arange(wl * hl) // wl
    ox, oy = col * 64, row * 64
    complete = (ox + 64 <= w) & (oy + 64 <= h)
    cols, rows = ((3, 2), (7, 4), (7, 4), (14, 8))[cls]
    logo = (((ox >= w - cols * 64) | (ox < cols * 64)) & (oy < rows * 64)) | (oy >= h - rows * 64)
    return wl, hl, col, row, complete, logo


def make_inputs(w, h, cls, seed, seq):
    """the records of every picture of a sequence -> list of dicts (me, stats, detect).  Variances stay below 16,384, as those of 8-bit pictures do"""
    rng = np.random.default_rng([seed, 24])
    wl, hl, col, row, complete, logo = geometry(w, h, cls)
    n = wl * hl
    # ---- what persists over the sequence: the kind of every LCU (0 flat, 1 medium, 2 strong), its logo block of edge units, whether it stands still ----
    if seq["strong"] or seq["medium"]:
        kind = np.zeros(n, int)
        for c, r in seq["medium"]:
            kind[r * wl + c] = 1
        for c, r in seq["strong"]:
            kind[r * wl + c] = 2
        drawn = False
    else:
        kind = rng.choice(3, n, p=(0.45, 0.2, 0.35))
        drawn = True
    block = np.where(kind > 0, rng.integers(0, 65536, n) | rng.integers(0, 65536, n) | 0x0660, rng.integers(0, 65536, n) & rng.integers(0, 65536, n))
    still = (kind > 0) | (rng.random(n) < 0.05)
    base64 = rng.integers(100, 12000, n)
    steady = rng.random(n) < 0.5
    recs = []
    for k, p in enumerate(seq["pics"]):
        r = np.random.default_rng([seed, 24, k])
        # ---- block statistics: the four 32x32 variances around a mean, spread by the kind; now and then a picture falls out of its kind ----
        kd = kind.copy()
        out = r.random(n) < (0.1 if drawn else 0.03)
        kd[out] = r.integers(0, 3, int(out.sum()))
        spread = np.where(kd == 2, r.integers(230, 700, n), np.where(kd == 1, r.integers(36, 215, n), r.integers(0, 30, n)))
        mean = r.integers(2000, 9000, n)
        stats = np.zeros(n, S.PA_LCU_STATS_DTYPE)
        stats["variance"] = r.integers(0, 2000, (n, 85))
        stats["y_mean"] = r.integers(0, 256, (n, 85))
        sign = np.array([1, -1, 1, -1])[r.permuted(np.tile(np.arange(4), (n, 1)), axis=1)]
        stats["variance"][:, 1:5] = mean[:, None] + sign * spread[:, None] + r.integers(-3, 4, (n, 4))
        stats["variance"][:, 0] = np.clip(base64 + np.where(steady, r.integers(-25, 26, n), r.integers(-4000, 4001, n)), 0, 16383)
        # ---- ME records: the vectors by the picture's motion, the logo blocks standing still; the 64x64 distortion around Part2's thresholds ----
        me = np.zeros(n, S.ME_LCU_DTYPE)
        mv = r.integers(-300, 301, (n, 85, 4))
        kind_of_motion = p["motion"]
        if kind_of_motion == "pan":
            mv[:, 0, 0], mv[:, 0, 1] = 96 + r.integers(-10, 11, n), r.integers(-7, 8, n)
        elif kind_of_motion == "tilt":
            mv[:, 0, 0], mv[:, 0, 1] = r.integers(-7, 8, n), -80 + r.integers(-10, 11, n)
        elif kind_of_motion == "still":
            mv[:, 0, :2] = r.integers(-3, 4, (n, 2))
        if kind_of_motion != "mixed":
            stray = r.random(n) < 0.08
            mv[stray, 0, :2] = r.integers(-200, 201, (int(stray.sum()), 2))
        mv[still, 0, :2] = r.integers(-17, 18, (int(still.sum()), 2))           # around Part1's 16
        me["pu"]["mv"] = mv
        me["pu"]["distortion"] = r.integers(0, 1 << 18, (n, 85, 3))
        me["pu"]["distortion"][:, 0, 0] = np.array((3000, 8191, 8192, 20479, 20480, 30000, 70000))[r.integers(0, 7, n)]
        me["pu"]["direction"], me["pu"]["total"] = 0, 1
        # ---- detector records: edge_cu as EdgeDetectionMeanLumaChroma16x16 leaves it - every fourth picture, complete potential-logo LCUs ----
        detect = np.zeros(n, LCU_DETECT_DTYPE)
        if (p["poc"] & 3) == 0:
            lost = np.where(kind == 2, 0, r.integers(0, 65536, n) & r.integers(0, 65536, n) & r.integers(0, 65536, n))
            detect["edge_cu"] = np.where(logo & complete, block & ~lost, 0)
        detect["homogeneous"] = r.random(n) < 0.5
        recs.append(dict(me=me, stats=stats, detect=detect))
    return recs


def case_inputs(name):
    w, h, cls, seed, seq = CASES[name]
    return make_inputs(w, h, cls, seed, seq)
