"""CPU-only: the restatement of the initial rate control's look-ahead stage (tests/irc_numpy.py) against what the REFERENCE's own functions computed on the
seeded records (tests/golden/irc_*.npz, tests/golden/make_irc_golden.py) - every field of every record - the proof that pass (a) of the stationary-edge stage
is a gather, and the conditions that make the fixtures worth having."""
import importlib.util
import os

import numpy as np
import pytest

import irc_numpy as N
import irc_records as R
import svtlib as S

CASES = sorted(R.CASES)
ARRAYS = (("checks", R.CHECKS_FIELDS), ("motion", R.MOTION_FIELDS), ("lcu", R.LCU_FIELDS), ("picture", R.PIC_FIELDS))


def load_case(name):
    g = np.load(os.path.join(S.GOLDEN_DIR, "irc_%s.npz" % name))
    assert str(g["case"][0]) == name
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def fixtures():
    return {name: load_case(name) for name in CASES}


def same(got, want, what):
    """every field of the six arrays of a sequence (or of a slice of one)"""
    for key, fields in ARRAYS:
        for f in fields:
            a, b = got[key][f], want[key][f]
            assert np.array_equal(a, b), (what, key, f, np.argwhere(np.asarray(a != b).reshape(a.shape[0], -1).any(1)).ravel()[:6].tolist())
    for key in ("stationary_edge", "pm_stationary_edge"):
        assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:6].tolist())


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(fixtures, name):
    g = fixtures[name]
    w, h, cls, seed, seq = R.CASES[name]
    lists = N.sequence_lists(seq)
    assert [ls["frames_to_check"] for ls in lists] == g["frames_to_check"].tolist()
    # the lists the restatement hands the device against what stood in the reference's queue where its walks passed
    assert [len(ls["hom"]) for ls in lists] == g["hom_walked"].tolist()
    for k, ls in enumerate(lists):
        first = k + int((seq["head0"] + k) % R.QUEUE_DEPTH == R.QUEUE_DEPTH - 1)
        assert ls["edge"] == [first + s for s in range(32) if int(g["edge_places"][k]) >> s & 1], (name, k)
    out = N.initial_rc(w, h, cls, seq, R.case_inputs(name), lists)
    same(out, g, name)
    for key in ("motion", "lcu", "picture"):
        assert not out[key]["pad"].any()
    assert not out["picture"]["pad0"].any()


def test_pass_a_in_place_equals_the_gather():
    """the in-place raster loop of pass (a) (Codec/EbSourceBasedOperationsProcess.c:1197-1244) clears an LCU exactly when its flag is 1 and none of its eight
    neighbours' flags was 1 before the pass: random flag maps of every size from 1x1 to 12x9, sparse and dense.  Eligibility: every LCU whose flag is 1 is
    eligible (the first loop sets a flag nowhere else), the others by chance"""
    rng = np.random.default_rng(24)
    maps = 0
    for wl in range(1, 13):
        for hl in range(1, 10):
            for density in (0.08, 0.25, 0.6):
                flag = (rng.random(wl * hl) < density).astype(np.uint8)
                eligible = (flag == 1) | (rng.random(wl * hl) < 0.5)
                assert np.array_equal(N.clear_isolated_loop(flag, eligible, wl, hl), N.clear_isolated_gather(flag, wl, hl)), (wl, hl, density, flag.tolist())
                maps += 1
    assert maps >= 200
    lone, pair = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0], np.uint8), np.array([1, 1, 0, 0, 0, 0, 0, 0, 1], np.uint8)
    assert not N.clear_isolated_gather(lone, 3, 3).any() and N.clear_isolated_gather(pair, 3, 3).tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]


def test_the_fixtures_are_not_vacuous(fixtures):
    """on the fixtures alone - the reference's records, and the places of its queue that the generator's driver saw its two walks pass: it is the reference that
    satisfies the conditions"""
    spec = importlib.util.spec_from_file_location("make_irc_golden", os.path.join(S.GOLDEN_DIR, "make_irc_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.assert_not_vacuous(fixtures)
    assert {R.CASES[name][2] for name in CASES} == {0, 1, 3}
    heads = [(R.CASES[name][4]["head0"] + k) % R.QUEUE_DEPTH for name in CASES for k in range(len(R.CASES[name][4]["pics"]))]
    assert R.QUEUE_DEPTH - 1 in heads and 0 in heads and 11 in heads            # the head at the last index, behind it, and elsewhere
    assert fixtures["tail_192x128"]["frames_to_check"].tolist() == [17] * 4 + list(range(16, 0, -1))
    last = R.CASES["ends_intra_128x64"][4]["pics"][-1]                           # an I picture leaves without a look-ahead
    assert last["slice_type"] == R.I and last["eos"] and fixtures["ends_intra_128x64"]["frames_to_check"][-1] == 1
    assert not fixtures["tail_192x128"]["checks"]["check2"][-1].any() and fixtures["tail_192x128"]["checks"]["check2"][:-1].all()
    for name in CASES:
        assert os.path.getsize(os.path.join(S.GOLDEN_DIR, "irc_%s.npz" % name)) < 100 * 1024


def test_the_window_lists_keep_their_bounds():
    """what the device job can hold: at most 4 counted entries, 16 homogeneity entries, 8 pan entries - for every case and the usual sequence"""
    for seq in [R.CASES[name][4] for name in CASES] + [R._usual_jobs()]:
        for p, ls in zip(seq["pics"], N.sequence_lists(seq)):
            assert len(ls["edge"]) <= 4 and len(ls["hom"]) <= 16 and len(ls["pan"]) <= 8 and 1 <= ls["frames_to_check"] <= 17
            assert ls["look_ahead"] == (not p["eos"]) and (ls["look_ahead"] or (ls["frames_to_check"] == 1 and not ls["edge"] + ls["hom"] + ls["pan"]))


def test_seeded_variances_stay_below_the_bound_of_8_bit_pictures():
    """the int product of two variances (Codec/EbInitialRateControlProcess.c:695) and the int sum of four squared differences
    (Codec/EbMotionEstimationProcess.c:527) do not overflow below 16,384"""
    for name in CASES:
        for rec in R.case_inputs(name):
            assert int(rec["stats"]["variance"][:, :5].max()) < 16384
