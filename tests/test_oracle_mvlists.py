"""CPU-only: the motion-vector candidate lists of P / B units at the ends of their input ranges - POC distances beyond the +-128 clips, scale factors and scaled
components at their clips, the rounding term of negative products, co-located list 1, no temporal candidate, ClipMV on 4096 x 2304 pictures - where no recorded
picture goes (tests/golden/md_*.npz: distances within [-4, 8], vectors up to 464).

tests/golden/mvlists_seeded.npz holds seeded single-unit jobs (tests/mvlists_jobs.py) and what the REFERENCE's own GenerateL0L1AmvpMergeLists and ChooseMVPIdx_V2
answered on them (oracle/ref_harness_mvlists.c, tests/golden/make_mvlists_golden.py).  Here:
  (a) the fixture holds every path the lists can take, counted by a plain model of the lists that must itself reproduce the fixture;
  (b) the CPU checker's text (svt-hevc_amd/csrc/md_logic.h: md_amvp_merge_lists, md_choose_mvp through svt_oracle_md_lists) gives the reference's outs;
  (c) where the reference is built: it reproduces the fixture, and checker and reference agree on a second seed of jobs that are not committed.
The register form of the same lists that the device's unit loop executes is pinned to the same fixture by tests/test_gpu_md_lists.py."""
import os

import numpy as np
import pytest

import mvlists_jobs as J
import svtlib as S


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(S.GOLDEN_DIR, "mvlists_seeded.npz"))
    jobs, pool, outs = g["jobs"], g["pool"], g["outs"]
    assert jobs.dtype == J.JOB_DTYPE and pool.dtype == J.TMVP_DTYPE and outs.dtype == J.OUT_DTYPE and len(outs) == len(jobs)
    return jobs, pool, outs


def check_ranges(jobs, pool):
    """the input ranges the jobs must stay inside: outside them the three texts divide by zero or the reference's 16-bit narrowings wrap"""
    assert 2000 <= len(jobs) <= 6000
    pn = jobs["picture_number"].astype(np.int64)
    for l in range(2):
        d = pn - jobs["ref_poc"][:, l].astype(np.int64)
        assert (d != 0).all() and (np.abs(d) <= 1000).all()
    col = np.where(jobs["slice_type"] == 0, jobs["colocated_pu_ref_list"], 0)
    assert (jobs["colocated_poc"] == jobs["ref_poc"][np.arange(len(jobs)), col]).all()
    for i in range(len(jobs)):
        for k in range(2):
            d = int(jobs[i]["colocated_poc"]) - pool[int(jobs[i]["pool"][k])]["ref_poc"].astype(np.int64)
            assert (d != 0).all() and (np.abs(d) <= 1000).all(), (i, k)
    assert int(jobs["pool"].max()) < len(pool) and np.isin(pool["available"], (0, 1)).all() and (pool["pred_dir"] <= 2).all()
    w, h, s = jobs["width"].astype(int), jobs["height"].astype(int), jobs["size"].astype(int)
    assert (w >= 72).all() and (h >= 72).all() and (w <= 4096).all() and (h <= 2304).all() and (w % 8 == 0).all() and (h % 8 == 0).all()
    assert np.isin(s, (8, 16, 32, 64)).all() and (jobs["ox"] % s == 0).all() and (jobs["oy"] % s == 0).all()
    assert (jobs["ox"] + s <= w).all() and (jobs["oy"] + s <= h).all()
    assert np.isin(jobs["slice_type"], (0, 1)).all() and np.isin(jobs["total_merge"], (2, 3, 5)).all() and (jobs["me_dir"] <= 2).all()
    p = jobs["slice_type"] == 1
    assert (jobs["me_dir"][p] == 0).all() and (jobs["nb"]["dir"][p] == 0).all() and (jobs["nb"]["dir"] <= 2).all() and np.isin(jobs["nb"]["avail"], (0, 1)).all()
    # both ends of int16 among the vectors of every kind
    for v in (jobs["nb"]["mv"], jobs["me_mv"], pool["mv"]):
        assert v.min() == -32768 and v.max() == 32767
    # partial LCUs at the right and at the bottom, units on the picture's right and bottom edge, at LCU corners, on the LCU's bottom edge
    assert ((w % 64 != 0) & (jobs["ox"] + s == w)).sum() >= 20 and ((h % 64 != 0) & (jobs["oy"] + s == h)).sum() >= 20
    assert ((jobs["ox"] % 64 == 0) & (jobs["oy"] % 64 == 0)).sum() >= 20 and (((jobs["ox"] + s) % 64 == 0) & ((jobs["oy"] + s) % 64 == 0)).sum() >= 20
    assert (((jobs["oy"] & 63) + s == 64) & (jobs["oy"] + s < h)).sum() >= 20
    assert (w == 4096).sum() >= 20 and (w == 72).sum() >= 20


def test_fixture_covers_every_path(fixture):
    """(a) read from the fixture alone: the ranges, and at least CONDITIONS[c] jobs on every path c - named by a model that reproduces the reference's outs"""
    jobs, pool, outs = fixture
    check_ranges(jobs, pool)
    model, flags = J.model_out_array(jobs, pool)
    J.compare_outs(jobs, model, outs, "the counting model against the fixture")
    counts = J.coverage(jobs, flags)
    for c in J.CONDITIONS:
        print("%-60s %5d" % (c, counts[c]))
    short = {c: n for c, n in counts.items() if n < J.CONDITIONS[c]}
    assert not short, short


def test_fixture_is_the_seeded_job_set(fixture):
    """the committed jobs are what the generator makes of its seeds: the fixture can be rebuilt, and a changed generator does not silently leave it behind"""
    jobs, pool, _ = fixture
    want_pool = J.make_pool(J.POOL_SEED)
    assert np.array_equal(pool, want_pool) and np.array_equal(jobs, J.make_jobs(J.SEED, J.COUNT, want_pool))


def test_checker_equals_reference_records(fixture):
    """(b) md_logic.h's lists and predictor choice on every job of the fixture"""
    jobs, pool, outs = fixture
    got = J.run_lists(S.load_oracle().svt_oracle_md_lists, jobs, pool)
    J.compare_outs(jobs, got, outs, "svt_oracle_md_lists against the reference's records")


def test_reference_reproduces_fixture_and_second_seed(fixture):
    """(c) the reference itself, where it is built"""
    ref = S.load_ref()
    if ref is None or not hasattr(ref, "svt_ref_mv_lists"):
        pytest.skip("oracle/_ref/libsvtref.so not built")
    jobs, pool, outs = fixture
    again = J.run_lists(ref.svt_ref_mv_lists, jobs, pool, returns=True)
    assert again.tobytes() == outs.tobytes()
    pool2 = J.make_pool(J.POOL_SEED + 1)
    jobs2 = J.make_jobs(J.SEED + 1, 3000, pool2)
    check_ranges(jobs2, pool2)
    want = J.run_lists(ref.svt_ref_mv_lists, jobs2, pool2, returns=True)
    got = J.run_lists(S.load_oracle().svt_oracle_md_lists, jobs2, pool2)
    J.compare_outs(jobs2, got, want, "svt_oracle_md_lists against the reference, second seed")
