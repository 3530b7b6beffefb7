"""Seeded input records of the mode decision's per-LCU controls (integration/svt_md_fill.h:svt_md_fill_lcu with DeriveContouringClass, Codec/EbModeDecisionConfiguration.c:395,
and ConfigureChroma, Codec/EbModeDecisionProcess.c:383) in the form the batched device entry svt_amd_md_controls_batch_launch takes them: what the batches in front of it
leave per picture - the mode-decision configuration's LCU records, block statistics, detector records, the source-based operations' LCU and picture records, the
initial rate control's LCU records and stationary-edge bytes, the AC energies - and the scalars the reference's host owns, drawn around the thresholds the rules
test (256 / 1024 / 2048 / 3072 and 100000000 for the energies; 50, 200 and 2 for the mean, the variance and the non-moving index).  Shared by the fixture generator
(tests/golden/make_mdctl_golden.py), the CPU suite and the GPU suite: the fixtures hold the case names and the reference's results only, the inputs are drawn again
from the seed."""
import numpy as np

import svtlib as S
from irc_records import IRC_LCU_DTYPE
from mdc_records import MDC_LCU_DTYPE, INVALID_AURA_STATUS, PICT_LCU_SWITCH, PICT_FULL85, PICT_FULL84, PICT_OPEN_LOOP, geometry, unit_validity
from pa_detect_numpy import LCU_DETECT_DTYPE
from sbo_records import SBO_LCU_DTYPE, SBO_PIC_DTYPE

MD_LCU_DTYPE = S.MD_LCU_DTYPE
CHECK_DTYPE = np.dtype([("bad_leaf_count", "<u4"), ("bad_leaf_list", "<u4"), ("md_mode", "<u4", 16), ("bad_chroma", "<u4"), ("tiles", "<u4"), ("first_bad", "<u4"),
                        ("first_kind", "<u4")])
assert MD_LCU_DTYPE.itemsize == 191 and CHECK_DTYPE.itemsize == 88
HEAD_BYTES = 171                        # leaf_count, leaf_index[85], leaf_split[85]: shared with SvtAmdMdcLcu
TAIL_FIELDS = tuple(f for f in MD_LCU_DTYPE.names[3:] if not f.startswith("pad"))
FLAG_FIELDS = ("restrict_intra_global_motion", "skip_small_cu", "cmplx_noise", "variance_below_200", "edge_block", "no_stop_split", "complexity_status_2", "is_complete")
ENERGIES = (0, 255, 256, 1023, 1024, 2047, 2048, 2500, 3071, 3072, 9000)
INCOMPLETE_ENERGY = 100000000           # what CalculateAcEnergy leaves for an LCU the picture does not cover (Codec/EbSourceBasedOperationsProcess.c:302)
I, P, B = 0, 1, 2


def job(slice_type=B, depth_mode=PICT_LCU_SWITCH, chroma_level=1, cls=0, pan=0, tilt=0, c422=0, tiles=(1, 1), mdc=True, irc=True, stationary="some", sticky="some",
        grass=20):
    """the scalars of a job and the knobs of make_inputs.  mdc False: no configuration records (depth_mode 1 / 2 only); irc False: neither initial-rate-control
    records nor energies; stationary / sticky: 'none' (NULL pointer) or 'some'"""
    return dict(slice_type=slice_type, depth_mode=depth_mode, chroma_level=chroma_level, cls=cls, pan=pan, tilt=tilt, c422=c422, tile_cols=tiles[0], tile_rows=tiles[1],
                mdc=mdc, irc=irc, stationary=stationary, sticky=sticky, grass=grass)


def _usual_jobs(cls=0, tiles=(1, 1)):
    """I, P and B pictures, every chroma level, pan and tilt, 4:2:2, grass on either side of 60, with and without configuration records (FULL84 and FULL85),
    with and without the initial rate control's records, the stationary-edge and the sticky bytes given and NULL"""
    return [job(B, PICT_LCU_SWITCH, 2, cls, tiles=tiles),
            job(B, PICT_LCU_SWITCH, 3, cls, pan=1, tiles=tiles, sticky="none"),
            job(P, PICT_LCU_SWITCH, 4, cls, tilt=1, tiles=tiles, grass=20),
            job(B, PICT_OPEN_LOOP, 4, cls, tiles=tiles, grass=61, stationary="none"),
            job(B, PICT_LCU_SWITCH, 5, cls, tiles=tiles),
            job(I, PICT_FULL84, 0, cls, tiles=tiles, mdc=False),
            job(I, PICT_FULL85, 1, cls, tiles=tiles, mdc=False, irc=False),
            job(P, PICT_FULL85, 2, cls, c422=1, tiles=tiles),
            job(B, PICT_FULL84, 2, cls, pan=1, tilt=1, tiles=tiles, irc=False, sticky="none", stationary="none"),
            job(B, PICT_LCU_SWITCH, 4, cls, pan=1, tiles=tiles)]


#          width, height, seed, jobs
CASES = {
    "one_64x64": (64, 64, 3, _usual_jobs()),                              # one LCU: an edge LCU, every tile flag set
    "partial_416x240": (416, 240, 5, _usual_jobs()),                      # partial right column and bottom row: edge LCUs by their origin
    "tiles_640x384": (640, 384, 7, _usual_jobs(cls=1, tiles=(2, 2))),     # 10 x 6 LCUs in 2 x 2 tiles, whole LCUs: the last column and row are no edge LCUs
    "uneven_704x640": (704, 640, 9, _usual_jobs(cls=2, tiles=(3, 4))),    # 11 x 10 LCUs in 3 x 4 tiles: the tile starts are 0, 3, 7 and 0, 2, 5, 7
    "class3_448x200": (448, 200, 11, _usual_jobs(cls=3, tiles=(7, 1))),   # class 3 forced on a small picture: no aura arm of no_stop_split; a tile per column
}


def random_leaves(rng, valid):
    """a leaf list as the configuration may leave it: a strictly ascending choice of valid units, at least one; the split flags anything"""
    n = len(valid)
    out = np.zeros(n, MDC_LCU_DTYPE)
    for i in range(n):
        units = np.flatnonzero(valid[i])
        keep = units[rng.random(len(units)) < rng.choice((0.1, 0.5, 1.0))]
        if len(keep) == 0:
            keep = units[:1]
        out["leaf_count"][i] = len(keep)
        out["leaf_index"][i, :len(keep)] = keep
        out["leaf_split"][i, :len(keep)] = rng.integers(0, 2, len(keep))
    return out


def make_inputs(w, h, seed, index, jb):
    """the records of job `index` of a case -> dict of arrays; an absent array is None"""
    rng = np.random.default_rng([seed, index, 25])
    wl, hl, col, row, complete, edge = geometry(w, h)
    n = wl * hl
    pick = lambda values, size: np.array(values)[rng.integers(0, len(values), size)]  # noqa: E731
    mdc = None
    if jb["mdc"]:
        mdc = random_leaves(rng, unit_validity(w, h))
        mdc["lcu_md_mode"] = rng.integers(1, 11, n) if jb["depth_mode"] == PICT_LCU_SWITCH else rng.integers(0, 11, n)   # kept under PICT_LCU_SWITCH only
        mdc["aura_status"] = pick((0, 0, 1, 1, INVALID_AURA_STATUS), n)
        mdc["pred64"], mdc["avc_partitioning"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
        mdc["lcu_score"], mdc["lcu_cost"] = rng.integers(0, 1 << 32, n), rng.integers(0, 256, n)
    stats = np.zeros(n, S.PA_LCU_STATS_DTYPE)
    stats["variance"] = rng.integers(0, 2000, (n, 85))
    stats["y_mean"] = rng.integers(0, 256, (n, 85))
    stats["variance"][:, 0] = pick((0, 199, 200, 201, 4000), n)
    stats["y_mean"][:, 0] = pick((0, 49, 50, 51, 200), n)
    detect = np.zeros(n, LCU_DETECT_DTYPE)
    detect["edge_block_num"] = pick((0, 0, 1, 5), n)
    detect["homogeneous"] = rng.random(n) < 0.5
    detect["edge_cu"], detect["sharp_edge"] = rng.integers(0, 65536, n), rng.integers(0, 2, n)
    sbo_lcu = np.zeros(n, SBO_LCU_DTYPE)
    sbo_lcu["high_luma"] = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 65536, n))
    sbo_lcu["high_chroma"] = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 65536, n))
    sbo_lcu["grass"], sbo_lcu["skin"] = rng.integers(0, 65536, n), rng.integers(0, 65536, n)
    sbo_lcu["non_moving_index"] = pick((0, 1, 2, 3, 255), n)
    sbo_lcu["zz_cost"] = rng.integers(0, 31, n)
    sbo_lcu["complex_lcu"] = rng.integers(0, 3, n)
    sbo_lcu["cmplx_status"] = pick((0, 4), n)
    sbo_lcu["isolated_non_homogeneous"] = rng.random(n) < 0.3
    sbo_lcu["cmplx_contrast"], sbo_lcu["failing_motion"] = rng.integers(0, 2, n), rng.integers(0, 2, n)
    sbo_pic = np.zeros(1, SBO_PIC_DTYPE)
    sbo_pic["grass_percentage"], sbo_pic["complete_lcu_count"] = jb["grass"], int(complete.sum())
    irc_lcu = energy = None
    if jb["irc"]:
        irc_lcu = np.zeros(n, IRC_LCU_DTYPE)
        irc_lcu["homogeneous_over_time"] = rng.random(n) < 0.7
        irc_lcu["var_of_var_over_time"], irc_lcu["motion_votes"] = rng.integers(0, 9000, n), rng.integers(0, 16, n)
        irc_lcu["similar_edge_count"] = rng.integers(0, 5, (n, 16))
        energy = pick(ENERGIES, (n, 5)).astype(np.uint64)
        big = rng.random((n, 5)) < 0.05
        energy[big] = rng.integers(1 << 32, 1 << 40, int(big.sum())).astype(np.uint64)     # beyond 32 bits: the comparison is 64 bits wide
        energy[~complete] = INCOMPLETE_ENERGY
    stationary = (rng.random(n) < 0.3).astype(np.uint8) * pick((1, 2, 3), n).astype(np.uint8) if jb["stationary"] == "some" else None
    sticky = np.where(rng.random(n) < 0.4, rng.integers(1, 4, n), 0).astype(np.uint8) if jb["sticky"] == "some" else None
    return dict(mdc_lcu=mdc, stats=stats, detect=detect, sbo_lcu=sbo_lcu, sbo_pic=sbo_pic, irc_lcu=irc_lcu, ac_energy=energy, stationary_edge=stationary, sticky=sticky)


def case_inputs(name):
    w, h, seed, jobs = CASES[name]
    return [make_inputs(w, h, seed, i, jb) for i, jb in enumerate(jobs)]


def conditions(rec, jb, sticky=True):
    """the four inputs of ConfigureChroma as the INPUTS give them (no rule of the levels) -> c0, c1, c2, c3 per LCU; aura status 128 without configuration records"""
    n = len(rec["stats"])
    st = rec["stationary_edge"] if rec["stationary_edge"] is not None else np.zeros(n, np.uint8)
    sk = rec["sticky"] if rec["sticky"] is not None and sticky else np.zeros(n, np.uint8)
    aura = rec["mdc_lcu"]["aura_status"] if rec["mdc_lcu"] is not None else np.full(n, INVALID_AURA_STATUS)
    high_luma, high_chroma = ((sk & 1) != 0) | (rec["sbo_lcu"]["high_luma"] != 0), ((sk & 2) != 0) | (rec["sbo_lcu"]["high_chroma"] != 0)
    c3 = (int(rec["sbo_pic"]["grass_percentage"][0]) > 60) | (aura == 1) | bool(jb["pan"])
    return st != 0, (rec["detect"]["homogeneous"] != 0) & high_chroma, ~high_luma, c3
