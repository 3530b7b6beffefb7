"""CPU-only, oracle only: the tap-matched planes of tests/inter_extremes.py reach the ends of the interpolation's 16-bit intermediates, and the oracle
(oracle/svt_oracle_mcp.c) computes there what a plain Python integer restatement of the two passes computes on the sign pattern.  The oracle's pin to
the reference at these ends is in tests/test_oracle_mcp.py (the matched cases), the device's in tests/test_gpu_inter_extremes.py."""
import ctypes as C

import numpy as np
import pytest

import inter_extremes as X

u32, vp = C.c_uint32, C.c_void_p
ROWS, COLS, OY, OX = 40, 48, 16, 16            # the block sits at (16, 16): room for every tap on every side


def decl(oracle):
    oracle.svt_oracle_mcp.argtypes = [C.c_int, C.c_int, C.c_int, u32, u32, vp, u32, vp, u32, u32, u32]
    oracle.svt_oracle_mcp.restype = None


def oracle_block(oracle, bps, chroma, raw, fx, fy, plane, n):
    out = np.zeros((n, n), np.int16 if raw else X.dtype_of(bps))
    oracle.svt_oracle_mcp(bps, chroma, raw, fx, fy, plane.ctypes.data + (OY * plane.shape[1] + OX) * bps, plane.shape[1], out.ctypes.data, n, n, n)
    return out


def test_planes_follow_the_tap_signs():
    """the generator against the definition, sample by sample, at a phase that is no multiple of the period"""
    for chroma, fx, fy in ((0, 2, 2), (0, 1, 3), (0, 0, 3), (1, 4, 4), (1, 7, 0), (1, 1, 6)):
        P, first = X.geometry(chroma)
        sx, sy = np.sign(X.taps_of(chroma, fx)), np.sign(X.taps_of(chroma, fy))
        for negative in (False, True):
            a = X.matched_plane(1, chroma, fx, fy, negative, 19, 23, 5, 3)
            for y in range(19):
                for x in range(23):
                    p = sx[(x - 5 - first) % P] * sy[(y - 3 - first) % P]
                    assert a[y, x] == (255 if (p < 0 if negative else p > 0) else 0), (chroma, fx, fy, negative, x, y)
            b = X.matched_plane(2, chroma, fx, fy, negative, 19, 23, 5, 3)
            assert np.array_equal(b == 1023, a == 255) and np.array_equal(b == 0, a == 0)
            m = X.matched_plane_msb(chroma, fx, fy, negative, 19, 23, 5, 3, 0)
            assert np.array_equal(m >> 2, a) and m.dtype == np.uint16
    m = X.matched_plane_msb(0, 2, 2, False, 64, 64, 0, 0, 0)
    assert sorted(set((m & 3).reshape(-1).tolist())) == [0, 1, 2, 3] and int(m.max()) == 1023


@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("chroma", [0, 1])
def test_oracle_reaches_the_ends_on_matched_planes(oracle, bps, chroma):
    decl(oracle)
    n = 8 if chroma else 16                     # at least one whole period of output phases
    maxv = X.maxv_of(bps)
    for fx, fy in X.positions(chroma):
        raws, unis = [], []
        for negative in (False, True):
            plane = X.matched_plane(bps, chroma, fx, fy, negative, ROWS, COLS, OX, OY)
            raw = oracle_block(oracle, bps, chroma, 1, fx, fy, plane, n)
            raws.append(raw)
            unis.append(oracle_block(oracle, bps, chroma, 0, fx, fy, plane, n))
            lo, hi, at_phase = X.restated_ends(bps, chroma, fx, fy, negative)
            assert (int(raw.min()), int(raw.max())) == (lo, hi), (fx, fy, negative)
            assert int(raw[0, 0]) == at_phase, (fx, fy, negative)
        top, bottom = int(raws[0].max()), int(raws[1].min())
        if not (fx and fy):                     # copy and 1-D: the analytic ends, from the taps alone
            want_bottom, want_top = X.analytic_ends_1d(bps, chroma, fx or fy)
            assert (bottom, top) == (want_bottom, want_top), (fx, fy)
            assert int(raws[0][0, 0]) == want_top and int(raws[1][0, 0]) == want_bottom, (fx, fy)
        # uni-prediction: the clip works at both ends (the - plane of the copy position is all zero: nothing lies under a negative tap)
        both = np.concatenate([u.reshape(-1) for u in unis])
        assert int(both.min()) == 0 and int(both.max()) == maxv, (fx, fy)
        assert int(unis[0][0, 0]) == maxv and int(unis[1][0, 0]) == 0, (fx, fy)


@pytest.mark.parametrize("bps,top,bottom", [(1, 24958, -25022), (2, 25055, -25072)])
def test_half_sample_ends_do_not_degenerate(oracle, bps, top, bottom):
    """(2,2) luma: the widest 2-D range.  The figures are those of the oracle on these planes; the bound +-24900 is what guards the generator."""
    decl(oracle)
    got = []
    for negative in (False, True):
        plane = X.matched_plane(bps, 0, 2, 2, negative, ROWS, COLS, OX, OY)
        got.append(oracle_block(oracle, bps, 0, 1, 2, 2, plane, 16))
    assert int(got[0].max()) > 24900 and int(got[1].min()) < -24900
    assert (int(got[0].max()), int(got[1].min())) == (top, bottom)


def test_one_dimensional_ends_are_the_analytic_ones():
    """88 * 255 - 8192 and -24 * 255 - 8192 for the half-sample filter, and their 10-bit forms after the >> 2"""
    assert X.analytic_ends_1d(1, 0, 2) == (-14312, 14248)
    assert X.analytic_ends_1d(2, 0, 2) == (-14330, 14314)
    assert X.analytic_ends_1d(1, 1, 4) == (-8 * 255, 72 * 255)


def driven_range(bps, chroma):
    """(first-pass min, max, raw min, max) the matched planes of every position drive through the two passes (restatement only)"""
    track = {"first": [], "raw": []}
    for fx, fy in X.positions(chroma):
        for negative in (False, True):
            X.restated_ends(bps, chroma, fx, fy, negative, track)
    first = track["first"] or [0]
    return min(first), max(first), min(track["raw"]), max(track["raw"])


def test_every_intermediate_fits_sixteen_bits():
    """restate() asserts that nothing needs the wrap; the first pass is driven to its own analytic ends by the 2-D planes"""
    for bps in (1, 2):
        lo, hi = X.analytic_ends_1d(bps, 0, 2)
        f0, f1, r0, r1 = driven_range(bps, 0)
        assert (f0, f1) == (lo, hi) and r0 < -24900 and r1 > 24900
        f0, f1, r0, r1 = driven_range(bps, 1)
        ends = [X.analytic_ends_1d(bps, 1, f) for f in range(1, 8)]
        assert (f0, f1) == (min(e[0] for e in ends), max(e[1] for e in ends))


def test_mode_decision_fixtures_choose_inter_on_matched_reference_pictures(oracle):
    """the precondition of the mode-decision cases of tests/test_gpu_inter_extremes.py, on the oracle alone: with the recorded reference pictures replaced by
    matched planes, inter candidates still win - with fractional vectors in at least 10 tested leaves and bi-predicted in at least 3 (the B fixture; the last
    case is a P picture and adds uni-predicted fractional winners) - so the device's dot-product cores decide these leaves' costs"""
    import os
    import svtlib as S
    from test_oracle_md_golden import oracle_md_picture
    for name, k, signs in X.MD_CASES:
        g = np.load(os.path.join(S.GOLDEN_DIR, "md_%s.npz" % name))
        out, _ = oracle_md_picture(oracle, g, k, X.md_matched_planes(g, k, signs))
        frac, bi = X.md_inter_winners(out)
        assert frac >= 10 and (bi >= 3 or int(g["pic"][k]["slice_type"]) == 1), (name, k, signs, frac, bi)
