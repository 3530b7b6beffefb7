"""CPU-only: the restatement of the batched source-based operations (tests/sbo_numpy.py) against what the REFERENCE's own functions computed on the seeded
records (tests/golden/sbo_*.npz, tests/golden/make_sbo_golden.py) - every field of every LCU and picture record - the condition that makes the fixtures worth
having, and the sticky parent flags of GrassSkinLcu as the reference's uncleared object shows them."""
import importlib.util
import os

import numpy as np
import pytest

import sbo_numpy as N
import sbo_records as R
import svtlib as S

CASES = sorted(R.CASES)


def load_case(name):
    g = np.load(os.path.join(S.GOLDEN_DIR, "sbo_%s.npz" % name))
    assert str(g["case"][0]) == name
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def fixtures():
    return {name: load_case(name) for name in CASES}


def restated(name):
    """every picture of a case through the restatement, on ONE object: the parent flags are carried from picture to picture"""
    w, h, rw, rh, seed, jobs = R.CASES[name]
    parents, out = None, []
    for jb, rec in zip(jobs, R.case_inputs(name)):
        if jb["slice_type"] == 0:
            rec = dict(rec, ref_stats=None)           # an I picture has no reference picture
        lcu, pic, parents = N.source_ops(w, h, rec, jb, parents)
        out.append((lcu, pic, parents))
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(fixtures, name):
    g = fixtures[name]
    for j, (lcu, pic, parents) in enumerate(restated(name)):
        for f in R.LCU_FIELDS:
            assert np.array_equal(lcu[f], g["lcu"][j][f]), (name, j, f, np.flatnonzero(lcu[f] != g["lcu"][j][f])[:6].tolist())
        for f in R.PIC_FIELDS:
            assert np.array_equal(pic[f], g["picture"][j][f]), (name, j, f, pic[f], g["picture"][j][f])
        assert np.array_equal(parents, g["parents"][j]), (name, j, "parents")
        assert not lcu["pad"].any() and not pic["pad"].any()


def test_the_fixtures_are_not_vacuous(fixtures):
    spec = importlib.util.spec_from_file_location("make_sbo_golden", os.path.join(S.GOLDEN_DIR, "make_sbo_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.assert_not_vacuous(fixtures)
    # what the cases are there for: I, P and B pictures, layers 0..2, referenced or not, windows of 0, 1 and 17, skip_ois_8x8 both ways - in every geometry
    for name in ("one_64x64", "interior_192x192", "plain_320x256", "partial_416x240", "pairs_704x640"):
        jobs = R.CASES[name][5]
        for key, values in (("slice_type", {0, 1, 2}), ("layer", {0, 1, 2}), ("ref", {0, 1}), ("zz_count", {0, 1, 17}), ("skip", {0, 1}), ("qpm", {0, 1})):
            assert {jb[key] for jb in jobs} == values, (name, key)
    assert all(jb["cls"] == 3 for jb in R.CASES["class3_256x192"][5])
    for name in CASES:
        assert os.path.getsize(os.path.join(S.GOLDEN_DIR, "sbo_%s.npz" % name)) < 16 * 1024


def test_parent_flags_are_sticky_on_one_object(fixtures):
    """two pictures recorded on one uncleared picture-control-set object: the second has neither grass nor skin, its parents still carry the first picture's"""
    name = "sticky_192x128"
    g = fixtures[name]
    w, h, rw, rh, seed, jobs = R.CASES[name]
    recs = R.case_inputs(name)
    first, second = g["lcu"][0], g["lcu"][1]
    assert first["grass"].any() and first["skin"].any() and not second["grass"].any() and not second["skin"].any()
    assert g["parents"][1][:, 0].any() and g["parents"][1][:, 1].any()                      # grass and skin parents outlive their picture
    assert np.array_equal(g["parents"][1][:, :2], g["parents"][0][:, :2])
    lcu0, _, p0 = N.source_ops(w, h, dict(recs[0], ref_stats=None), jobs[0], None)
    lcu1, _, carried = N.source_ops(w, h, recs[1], jobs[1], p0)
    _, _, fresh = N.source_ops(w, h, recs[1], jobs[1], None)
    assert np.array_equal(carried, g["parents"][1]) and not np.array_equal(fresh, g["parents"][1])
    assert not fresh[:, :2].any()                                                            # the per-picture value: what the device's masks give
    assert np.array_equal(lcu1["grass"], second["grass"])


def test_no_complete_lcu_gives_zero_averages():
    """item 10: the reference leaves stale averages; the restatement (and the device) write 0 with complete_lcu_count 0"""
    jb = R.job(R.B, 1, 1, 3, qpm=1)
    rec = R.make_inputs(48, 40, 1, 1, 23, 0, jb)
    lcu, pic, _ = N.source_ops(48, 40, rec, jb)
    assert pic["complete_lcu_count"] == 0 and pic["non_moving_index_average"] == 0 and pic["zz_cost_average"] == 0 and pic["low_motion_content"] == 1
    assert pic["processed_leaf_count"].tolist()[0] == 0 and pic["intra_complexity_avg"][0] == 0
