"""CPU-only companion of tests/test_gpu_intra_ref_extremes.py: the oracle alone on the cases of tests/intra_ref_extremes.py.  The threshold grid discriminates -
the smoothing flag changes the oracle's reconstruction of the unit exactly where the bilinear filter must fire - the size gate holds, every named mask makes
the neighbour groups unavailable that it claims, and the committed threshold fixtures hold the classes they were selected for."""
import os

import numpy as np
import pytest

import intra_ref_extremes as X
import svtlib as S


@pytest.mark.parametrize("bps", [1, 2])
def test_the_flag_changes_the_grid_exactly_inside_both_thresholds(oracle, bps):
    cases = [c for c in X.grid_cases(bps) if c["strong"]]
    assert len(cases) == 16 * len(X.GRID_MODES) and len(X.grid_cases(bps)) == 20 * len(X.GRID_MODES)
    on, off = X.picture(oracle, cases)["want"], X.picture(oracle, [dict(c, strong=0) for c in cases])["want"]
    t, fires = X.thr_of(bps), 0
    for c, a, b in zip(cases, on, off):
        _, dl, dt, mode, _ = c["tag"]
        assert (int(c["left"][0][63]) + int(c["tl"][0]) - 2 * int(c["left"][0][31]), int(c["tl"][0]) + int(c["top"][0][63]) - 2 * int(c["top"][0][31])) == (dl, dt)
        want = abs(dl) < t and abs(dt) < t and mode not in X.UNFILTERED_32
        ya, yb = X.first_unit(c, a), X.first_unit(c, b)
        assert (not np.array_equal(ya[0], yb[0])) == want, (c["tag"], int((ya[0] != yb[0]).sum()))
        assert np.array_equal(ya[1], yb[1]) and np.array_equal(ya[2], yb[2]), c["tag"]
        fires += want
    assert fires == 4 * (len(X.GRID_MODES) - 3)


@pytest.mark.parametrize("bps", [1, 2])
def test_the_flag_changes_nothing_at_16x16(oracle, bps):
    cases = X.gate_cases(bps)
    want = X.picture(oracle, cases)["want"]
    by = {c["tag"]: r for c, r in zip(cases, want)}
    assert len(by) == len(cases) == 8 * len(X.GRID_MODES)
    for (kind, dl, dt, mode, strong), r in by.items():
        if strong:
            other = by[(kind, dl, dt, mode, 0)]
            for f in ("rec_y", "rec_cb", "rec_cr", "coeff_y"):
                assert np.array_equal(r[f], other[f]), (dl, dt, mode, f)
    # ... while the same borders are flat enough for the gate to matter: read as the sides of a 32x32 unit they would fire
    for c in cases:
        assert abs(int(c["left"][0][31]) + int(c["tl"][0]) - 2 * int(c["left"][0][15])) < X.thr_of(bps)


def constant(blocks, values):
    return all((b == v).all() for b, v in zip(blocks, values))


@pytest.mark.parametrize("bps", [1, 2])
def test_masks_make_unavailable_what_they_claim(oracle, bps):
    cases = X.mask_cases(bps)
    named = {c["tag"][1:]: c for c in cases if c["tag"][1] != "random"}
    mid = 128 if bps == 1 else 512
    for size in (32, 16, 8):
        n = size
        pu = lambda name: (named[(name, size, 1)], X.oracle_pu(oracle, bps, X.job_of(named[(name, size, 1)])))
        c, p = pu("all_inter")
        assert constant(p, [mid] * 3) and X.substituted(c) is None
        c, p = pu("corner_only")
        assert constant(p, c["tl"])
        c, p = pu("bottom_left_group_only")
        assert constant(p, [c["left"][0][2 * n - 1], c["left"][1][n - 1], c["left"][2][n - 1]])
        c, p = pu("last_top_right_group_only")
        assert constant(p, [c["top"][0][2 * n - 1], c["top"][1][n - 1], c["top"][2][n - 1]])
        c, p = pu("all_but_corner")
        for q, r in zip(p, X.oracle_pu(oracle, bps, X.job_of(dict(c, constrained=0, tl=c["left"][:, 0])))):
            assert np.array_equal(q, r)
        c, p = pu("left_inter_top_intra")
        s = X.substituted(c)
        assert all((s["left"][k][:2 * n >> (k > 0)] == c["tl"][k]).all() for k in range(3))
    # every mask, the random ones included: the prediction is that of the substituted neighbourhood with every group available
    for c in cases:
        s = X.substituted(c)
        if s is not None:
            for q, r in zip(X.oracle_pu(oracle, bps, X.job_of(c)), X.oracle_pu(oracle, bps, X.job_of(s))):
                assert np.array_equal(q, r), c["tag"]
    # the flat-left pair at 32x32: the left side is flat by substitution and the top side decides - one step inside it fires, on the threshold it does not
    t = X.thr_of(bps)
    for dt, fires in ((t - 1, True), (t, False)):
        c = named[("left_inter_top_intra", 32, dt, 1)]
        a, b = X.oracle_pu(oracle, bps, X.job_of(c))[0], X.oracle_pu(oracle, bps, X.job_of(dict(c, strong=0)))[0]
        assert (not np.array_equal(a, b)) == fires, dt


@pytest.mark.parametrize("bps", [1, 2])
def test_constrained_cases_differ_from_their_controls(oracle, bps):
    cases = X.mask_cases(bps)
    want = X.picture(oracle, cases)["want"]
    differ = same = 0
    for k in range(0, len(cases), 2):
        c, ctl = cases[k], cases[k + 1]
        assert c["constrained"] == 1 and ctl["constrained"] == 0 and c["tag"][:-1] == ctl["tag"][:-1]
        g = c["size"] // 2
        hidden = (c["mode_left"][:g] == 1).any() or (c["mode_top"][:g] == 1).any() or c["mode_tl"] == 1
        a, b = X.first_unit(c, want[k]), X.first_unit(ctl, want[k + 1])
        eq = all(np.array_equal(p, q) for p, q in zip(a, b))
        if c["tag"][1] == "random" or len(c["tag"]) == 5:       # a random mode may read none of the hidden groups, and mode 34 of the flat-left pair reads the top side
            # alone (on the threshold [1 2 1] stays with and without the left side): then the two predictions are one
            hidden = any(not np.array_equal(p, q) for p, q in zip(X.oracle_pu(oracle, bps, X.job_of(c)), X.oracle_pu(oracle, bps, X.job_of(ctl))))
        assert eq == (not hidden), c["tag"]
        differ, same = differ + (not eq), same + eq
    assert differ >= 45


@pytest.mark.parametrize("strong,constrained", [(1, 0), (0, 1)])
def test_random_pictures_take_the_flags(oracle, strong, constrained):
    """random_picture / random_inter_picture of tests/test_gpu_encodepass.py pass both flags into every work record; the defaults are those of before"""
    from test_gpu_encodepass import random_inter_picture, random_picture
    works, _ = random_picture(oracle, 136, 72, 30, 3, constrained=constrained, strong=strong)
    assert (works["strong_smoothing"] == strong).all() and (works["constrained_intra"] == constrained).all()
    works, _, _, _ = random_inter_picture(oracle, 136, 72, 30, 3, constrained=constrained, strong=strong)
    assert (works["strong_smoothing"] == strong).all() and (works["constrained_intra"] == constrained).all()
    works, _ = random_picture(oracle, 136, 72, 30, 3)
    assert (works["strong_smoothing"] == 1).all() and (works["constrained_intra"] == 0).all()


def test_constrained_b_pictures_hold_mixed_and_empty_neighbourhoods(oracle):
    """the pictures of test_encode_picture_constrained_intra_matches_oracle, counted from the work records and the oracle's mode map alone"""
    from test_gpu_encodepass import CONSTRAINED_PICTURES, constrained_neighbourhoods, random_inter_picture
    for w, h, qp, seed, kw in CONSTRAINED_PICTURES:
        works, _, _, _ = random_inter_picture(oracle, w, h, qp, seed, constrained=1, **kw)
        mixed, empty, intra = constrained_neighbourhoods(works, w, h)
        assert mixed >= 20 and empty >= 1, (w, h, seed, mixed, empty, intra)


def test_threshold_fixtures_hold_their_classes():
    """tests/golden/intra_thr_*.npz (tests/golden/make_intra_golden.py, THR_CASES): records of the reference on and next to the decision - in each fixture, so at
    each depth, at least one where the filter fires with the larger second difference at thr - 1 (A), and one a step outside on the left (B) and one a step
    outside on the top side (C) alone, where it must not"""
    from test_oracle_intra_golden import CASES, THR_CASES
    biggest = max(os.path.getsize(os.path.join(S.GOLDEN_DIR, "intra_%s.npz" % n)) for n in CASES if n not in THR_CASES)
    depths = set()
    for name in THR_CASES:
        assert name in CASES
        path = os.path.join(S.GOLDEN_DIR, "intra_%s.npz" % name)
        g = dict(np.load(path))
        bps = 2 if "10" in name.split("_")[1] else 1
        assert (g["bytes_per_sample"] == bps).all() and (g["size"] == 32).all() and (g["strong_smoothing"] == 1).all()
        cls = X.smoothing_classes(g)
        assert cls["available"].all() and (cls["fired"] | cls["B"] | cls["C"]).all()          # nothing else was kept
        counts = {k: int(cls[k].sum()) for k in ("fired", "A", "B", "C")}
        assert min(counts.values()) >= 1, (name, counts)
        assert os.path.getsize(path) < biggest
        depths.add(bps)
    assert depths == {1, 2}
