"""Tap-matched worst-case reference samples for the inter-prediction interpolation, shared by tests/test_inter_extremes_cpu.py, the matched cases of
tests/test_oracle_mcp.py and tests/test_gpu_inter_extremes.py.  numpy only: no library, no GPU.

The interpolation of H.265 8.5.3.3.3 is a separable filter whose taps have both signs.  A plane that holds the maximum under every positive tap and 0
under every negative one drives the filter to the top of its range, the complementary plane to the bottom; a random plane reaches half of the 2-D range
and a one-sample checker none of it (the even and the odd taps of the half-sample filter both sum to 32).  matched_plane() builds such planes for any
fractional position; restate() is a plain-integer restatement of the two passes on them that no C code takes part in."""
import numpy as np

# H.265 tables 8-11 (luma, quarter samples) and 8-12 (chroma, eighth samples); a zero fraction is the single tap 64 = +1 after its shift
LUMA_TAPS = [[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]]
CHROMA_TAPS = [[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4], [-2, 10, 58, -2]]


def maxv_of(bps):
    return 255 if bps == 1 else 1023


def dtype_of(bps):
    return np.uint8 if bps == 1 else np.uint16


def taps_of(chroma, frac):
    return CHROMA_TAPS[frac & 7] if chroma else LUMA_TAPS[frac & 3]


def geometry(chroma):
    """(period P = number of taps, offset `first` of the first tap from the output sample)"""
    return (4, -1) if chroma else (8, -3)


def positions(chroma):
    n = 8 if chroma else 4
    return [(fx, fy) for fy in range(n) for fx in range(n)]


def matched_mask(chroma, fx, fy, negative, rows, cols, x0, y0):
    """True where the sample at (x, y) lies under taps of (fx, fy) whose signs multiply to + (negative: to -) for an output sample at (x0, y0) - and,
    the pattern having the period of the filter length, for every output sample congruent to it.  Zero taps match in neither plane."""
    P, first = geometry(chroma)
    sx, sy = np.sign(taps_of(chroma, fx)), np.sign(taps_of(chroma, fy))
    px = sx[(np.arange(cols) - x0 - first) % P]
    py = sy[(np.arange(rows) - y0 - first) % P]
    prod = py[:, None] * px[None, :]
    return prod < 0 if negative else prod > 0


def matched_plane(bps, chroma, fx, fy, negative, rows, cols, x0, y0):
    """rows x cols samples: the maximum where matched_mask() holds, 0 elsewhere"""
    return np.where(matched_mask(chroma, fx, fy, negative, rows, cols, x0, y0), maxv_of(bps), 0).astype(dtype_of(bps))


def matched_plane_msb(chroma, fx, fy, negative, rows, cols, x0, y0, seed):
    """10-bit samples whose upper 8 bits are the 8-bit matched plane and whose lower two bits are random: for the entry that predicts in 8 bits from
    the 8 MSBs of 16-bit reference pictures.  Rounding instead of truncating turns 255.75 into 256, filtering the 10-bit value sees the low bits."""
    low = np.random.default_rng([31, chroma, fx, fy, int(negative), seed]).integers(0, 4, (rows, cols))
    return ((matched_plane(1, chroma, fx, fy, negative, rows, cols, x0, y0).astype(np.int64) << 2) | low).astype(np.uint16)


def int16_exact(v, what):
    """the specification wraps here (the reference stores an int16); on samples of the nominal range nothing may need to"""
    assert -32768 <= v <= 32767, (what, v)
    return v


def restate(bps, chroma, fx, fy, sample, x, y, track=None):
    """The raw (bi-prediction) output sample at (x, y) in plain Python integers: horizontal pass into 16-bit intermediates, vertical pass on them.
    sample(x, y) -> int.  s1 = 0 / 2 is the first-pass shift of 8- / 10-bit samples, B = 8192 the bias that centres the intermediates (0 for 8-bit chroma).
    track: optional dict whose "first" / "raw" lists collect every first-pass intermediate and every output."""
    P, first = geometry(chroma)
    tx, ty = taps_of(chroma, fx), taps_of(chroma, fy)
    s1, B = (0 if bps == 1 else 2), (8192 if (bps == 2 or not chroma) else 0)
    if not fx and not fy:
        v = int16_exact((sample(x, y) << (6 - s1)) - B, "copy")
    elif not fx or not fy:
        s = sum((tx[k] * sample(x + first + k, y)) if fx else (ty[k] * sample(x, y + first + k)) for k in range(P))
        v = int16_exact((s - (B << s1)) >> s1, "1-D")
    else:
        acc = 0
        for j in range(P):
            hs = sum(tx[k] * sample(x + first + k, y + first + j) for k in range(P))
            t = int16_exact((hs - (B << s1)) >> s1, "first pass")
            if track is not None:
                track["first"].append(t)
            acc += ty[j] * t
        v = int16_exact(acc >> 6, "2-D")
    if track is not None:
        track["raw"].append(v)
    return v


def restated_ends(bps, chroma, fx, fy, negative, track=None):
    """(smallest, largest, value at the matched phase) of the raw output over one period of output phases on the matched plane of (fx, fy), computed on
    the sign pattern itself (no plane is built)"""
    P, first = geometry(chroma)
    sx, sy = np.sign(taps_of(chroma, fx)).tolist(), np.sign(taps_of(chroma, fy)).tolist()
    maxv = maxv_of(bps)

    def sample(x, y):
        p = sx[(x - first) % P] * sy[(y - first) % P]
        return maxv if (p < 0 if negative else p > 0) else 0

    vals = [[restate(bps, chroma, fx, fy, sample, x, y, track) for x in range(P)] for y in range(P)]
    flat = [v for row in vals for v in row]
    return min(flat), max(flat), vals[0][0]


def analytic_ends_1d(bps, chroma, frac):
    """(bottom, top) of the raw 1-D output: every negative / every positive tap on the maximum"""
    t = taps_of(chroma, frac)
    s1, B = (0 if bps == 1 else 2), (8192 if (bps == 2 or not chroma) else 0)
    pos, neg = sum(v for v in t if v > 0), sum(v for v in t if v < 0)
    return (neg * maxv_of(bps) - (B << s1)) >> s1, (pos * maxv_of(bps) - (B << s1)) >> s1


# ---- mode-decision fixtures on substituted reference pictures ----------------------------------------------------------
# (fixture, picture, signs of the planes of list 0 and list 1).  The recorded 192x128 and 200x136 fixtures are P pictures (list 0 only): md_p_objects_320x192 is the
# smallest recorded B picture, and on its picture 2 inter candidates win with fractional vectors AND bi-predicted with + in list 0 and - in list 1.  The average of a
# plane and its complement is flat, though, and an error that has opposite signs under 0 and under the maximum cancels in it; so the same fixture runs with + in both
# lists and with - in both (picture 1: uni- and bi-predicted winners), where the two lists add up instead, and md_b_xc_binary_200x136 picture 2 adds uni-predicted
# fractional winners from the + planes alone.  tests/test_inter_extremes_cpu.py asserts the winners' counts on the oracle.
MD_CASES = [("p_objects_320x192_m8_ld", 2, "+-"), ("p_objects_320x192_m8_ld", 1, "++"), ("p_objects_320x192_m8_ld", 1, "--"), ("b_xc_binary_200x136_m8_q51", 2, "+-")]


def md_matched_planes(g, k, signs="+-"):
    """[[y, cb, cr], [y, cb, cr]] in the layout of picture k's recorded reference pictures: (2,2) luma and (4,4) chroma matched planes, phase (0,0) at the picture
    origin; signs[l] == "-": the complementary plane in list l"""
    sy, sc, ox, oy = (int(v) for v in g["ref_geom"][k][:4])
    out = []
    for l in range(2):
        neg = signs[l] == "-"
        rows_y, rows_c = g["ref%d_y" % l][k].size // sy, g["ref%d_cb" % l][k].size // sc
        out.append([matched_plane(1, 0, 2, 2, neg, rows_y, sy, ox, oy).reshape(g["ref%d_y" % l][k].shape)] +
                   [matched_plane(1, 1, 4, 4, neg, rows_c, sc, ox // 2, oy // 2).reshape(g["ref%d_%s" % (l, c)][k].shape) for c in ("cb", "cr")])
    return out


def md_inter_winners(out):
    """(inter winners with a fractional vector in a used list, bi-predicted inter winners) among the tested leaves of a picture's decisions"""
    inter = (out["tested"] == 1) & (out["pred_mode"] == 1)
    frac = np.zeros_like(inter)
    for l in range(2):
        used = inter & ((out["inter_dir"] == l) | (out["inter_dir"] == 2))
        frac |= used & (((out["mv"][..., l, 0] & 3) != 0) | ((out["mv"][..., l, 1] & 3) != 0))
    return int(frac.sum()), int((inter & (out["inter_dir"] == 2)).sum())
