"""CPU-only: the restatement of the mode-decision configuration (tests/mdc_numpy.py) against what the REFERENCE's own functions computed on the seeded
records (tests/golden/mdc_*.npz, tests/golden/make_mdc_golden.py) - every field of every LCU and picture record - and the conditions that make the fixtures
worth having."""
import importlib.util
import os

import numpy as np
import pytest

import mdc_numpy as N
import mdc_records as R
import svtlib as S

CASES = sorted(R.CASES)


def load_case(name):
    g = np.load(os.path.join(S.GOLDEN_DIR, "mdc_%s.npz" % name))
    assert str(g["case"][0]) == name
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def fixtures():
    return {name: load_case(name) for name in CASES}


def tables(g, j):
    """the SAD lambda and splitFlagBits[0], [3] the reference's tables gave picture j of a fixture"""
    return int(g["lambda_"][j]), g["split_bits"][j].tolist()


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(fixtures, name):
    g = fixtures[name]
    w, h, seed, jobs = R.CASES[name]
    for j, (jb, rec) in enumerate(zip(jobs, R.case_inputs(name))):
        lcu, pic, _ = N.md_config(w, h, rec, jb, *tables(g, j))
        for f in R.LCU_FIELDS:
            assert np.array_equal(lcu[f], g["lcu"][j][f]), (name, j, f, np.flatnonzero((lcu[f] != g["lcu"][j][f]).reshape(lcu.size, -1).any(1))[:6].tolist())
        for f in R.PIC_FIELDS:
            assert np.array_equal(pic[f], g["picture"][j][f]), (name, j, f, pic[f], g["picture"][j][f])
        assert not lcu["pad"].any() and not lcu["pad0"].any() and not pic["pad"].any() and not pic["pad0"].any()


def test_the_fixtures_are_not_vacuous(fixtures):
    spec = importlib.util.spec_from_file_location("make_mdc_golden", os.path.join(S.GOLDEN_DIR, "make_mdc_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.assert_not_vacuous(fixtures)
    # what the cases are there for, in every geometry that runs the usual jobs
    for name in ("one_64x64", "aura_192x192", "whole_256x128", "partial_416x240", "many_704x640"):
        jobs = R.CASES[name][3]
        for key, values in (("slice_type", {1, 2}), ("layer", {0, 1, 2, 3}), ("ref", {0, 1}), ("enc_mode", {3, 5, 7, 8, 9, 11}), ("qp", {20, 30, 38, 39, 51}),
                            ("noise", {1, 2, 3, 4, 5, 6, 7}), ("pan", {0, 1}), ("tilt", {0, 1}), ("cu8", {0, 1}), ("depth_mode", {0, 1, 2, 3}),
                            ("stationary", {"none", "some"})):
            assert {jb[key] for jb in jobs} == values, (name, key)
    assert {R.CASES[name][3][0]["cls"] for name in CASES} == {0, 2, 3}
    assert all(jb["cls"] == 3 for jb in R.CASES["whole_256x128"][3]) and all(jb["cls"] == 3 for jb in R.CASES["class3_704x640"][3][1:])
    for name in CASES:
        assert os.path.getsize(os.path.join(S.GOLDEN_DIR, "mdc_%s.npz" % name)) < 100 * 1024


def test_score_spans_lie_on_both_sides_of_the_32_bit_product():
    """maxToMinScore * scoreTh (:1431) is a 32-bit product: the fixtures hold pictures whose span times 100 fits 32 bits, and pictures whose scores
    DeriveLcuScore's unsigned differences threw to the top of the range, so that the product wraps"""
    spans = []
    for name in ("many_704x640", "class3_704x640", "partial_416x240"):
        g = load_case(name)
        p = g["picture"][g["picture"]["budget"] != 0]
        spans += ((p["lcu_max_score"].astype(np.int64) - p["lcu_min_score"]) & 0xFFFFFFFF).tolist()
    assert any(s > 0xFFFFFFFF // 100 for s in spans) and any(0 < s <= 0xFFFFFFFF // 100 for s in spans), spans


def test_leaf_lists_are_cut_to_leaf_count(fixtures):
    for name, g in fixtures.items():
        lcu = g["lcu"]
        behind = np.arange(85)[None, None, :] >= lcu["leaf_count"][:, :, None]
        assert not lcu["leaf_index"][behind].any() and not lcu["leaf_split"][behind].any(), name


def test_the_minus_one_thresholds_enter_as_unsigned():
    """scoreTh starts at ~0 = -1 and multiplies as 0xFFFFFFFF (:1431): where no threshold of DeriveDefaultSegments stands, the interval is chosen by
    numberOfSegments alone, and the threshold leaves the loop as 0 (MAX(-1 - 1, 0) while under-shooting, -1 + 1 while over-shooting)"""
    name = "many_704x640"
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    for j, jb in enumerate(jobs):
        if jb["depth_mode"] != R.PICT_LCU_SWITCH:
            continue
        th, nseg = g["picture"]["score_th"][j], int(g["picture"]["number_of_segments"][j])
        assert (th[5:] == -1).all() and (th[nseg - 1:5] == 0).all(), (j, th.tolist(), nseg)


def test_picture_wide_modes_write_no_budget():
    name = "partial_416x240"
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    valid = R.unit_validity(w, h)
    for j, jb in enumerate(jobs):
        lcu, pic = g["lcu"][j], g["picture"][j]
        if jb["depth_mode"] == R.PICT_FULL85:
            assert np.array_equal(lcu["leaf_count"], valid.sum(1))
        elif jb["depth_mode"] == R.PICT_FULL84:
            assert np.array_equal(lcu["leaf_count"], valid[:, 1:].sum(1))
        elif jb["depth_mode"] == R.PICT_BDP:
            assert not lcu["leaf_count"].any() and pic["average_qp"] == jb["qp"]
