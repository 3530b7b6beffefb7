"""-m gpu: motion estimation where the other GPU tests do not go - saturated pictures (every sample 0 or 255: block SADs at the largest value their
fields and the packed 16-bit lanes of the full-pel search hold, half-pel filters clipped at both ends), the smallest pictures a slot accepts (HME regions,
search area and search-centre clamps all larger than the picture, an only / last LCU 8 samples wide or high), and batches whose jobs differ in picture size,
controls and list count (k_me / k_ois read everything per job; the launchers size grid and LDS by the batch maximum).  Every comparison is bit-exact against
the CPU oracle; tests/golden/me_x_*.npz pin the oracle to the reference on the same saturated clips."""
import ctypes as C

import numpy as np
import pytest

import svtlib as S
from gpu_util import default_params, me_picture, read_plane, upload
from test_gpu_me import VARIANTS
from test_gpu_me_lds import CASES, LDS_PER_CU, lds_bytes
from test_gpu_ois import VARIANTS as OIS_VARIANTS, mk_params, same

pytestmark = pytest.mark.gpu

SEED = 5
# the 17 control sets: test_gpu_me.VARIANTS, the layout corners of test_gpu_me_lds.CASES, and the reference's own largest search area with the SSD arrays and
# two lists in the search kernel's LDS pool
CONTROLS = list(VARIANTS) + [kw for _, _, _, kw in CASES] + [
    dict(num_lists=2, temporal_layer_index=1, fractional_search_method=2, fractional_search_model=0, fractional_search_64x64=1, cu8x8_mode=0,
         search_area_width=64, search_area_height=64)]
assert len(CONTROLS) == 17
SATURATED = ["x_whiteblack", "x_binary", "x_stripes"]
MAX_SAD_64 = 2 * 32 * 64 * 255  # 1,044,480: the largest value the 64x64 SAD takes

_clips, _wants = {}, {}


def clip(oracle, kind, w, h, seed=SEED):
    """Frames t = 0, 1, 2 of a clip and the oracle's pictures of them, built once."""
    key = (kind, w, h, seed)
    if key not in _clips:
        frames = [S.gen_luma(kind, w, h, t, seed) for t in range(3)]
        _clips[key] = (frames, [S.OraclePicture(oracle, f) for f in frames])
    return _clips[key]


def oracle_me(oracle, kind, w, h, p, seed=SEED, key=None):
    """The oracle's records of picture t = 1 against t = 0 (and t = 2), computed once per `key`."""
    k = (kind, w, h, seed, key)
    if key is None or k not in _wants:
        _, pics = clip(oracle, kind, w, h, seed)
        want = S.oracle_me_picture(oracle, p, pics[1], pics[0], pics[2] if p.num_lists == 2 else None)
        if key is None:
            return want
        want.setflags(write=False)
        _wants[k] = want
    return _wants[k]


def compare_all(got, want, p, what):
    """compare_me, the HME centres and search sizes of test_me_matches_oracle, and for two lists every field of the record (test_gpu_me_lds)."""
    S.compare_me(got, want, p.num_lists, what)
    for k in ("hme_center_x", "hme_center_y", "search_w", "search_h"):
        assert np.array_equal(got[k][:, :p.num_lists], want[k][:, :p.num_lists]), (what, k)
    if p.num_lists == 2:
        for k in S.ME_LCU_DTYPE.names:
            if k != "pu":
                assert np.array_equal(got[k], want[k]), (what, k)
        assert np.array_equal(got["pu"]["mv"], want["pu"]["mv"]) and np.array_equal(got["pu"]["total"], want["pu"]["total"]), what


def search_and_compare(product, gpu_ctx, oracle, kind, w, h, ci):
    frames, _ = clip(oracle, kind, w, h)
    for s_, f in enumerate(frames):
        upload(product, gpu_ctx, s_, f)
    p = default_params(w, h, **CONTROLS[ci])
    if ci == 16:
        assert 0 < lds_bytes(product, p, 1) <= LDS_PER_CU
    want = oracle_me(oracle, kind, w, h, p, key=ci)
    got = me_picture(product, gpu_ctx, p, 1, [0, 2])
    compare_all(got, want, p, "%s %dx%d controls %d" % (kind, w, h, ci))
    return want


# ---- a. saturated pictures ----

@pytest.mark.parametrize("ci", range(len(CONTROLS)))
@pytest.mark.parametrize("kind", SATURATED)
def test_me_matches_oracle_on_saturated_pictures(product, gpu_ctx, oracle, kind, ci):
    want = search_and_compare(product, gpu_ctx, oracle, kind, 192, 128, ci)
    if kind == "x_whiteblack" and ci == 0:  # a white picture searched in a black one: the 64x64 SAD field at its maximum in every LCU
        assert (want["best_sad"][:, 0, 0] == MAX_SAD_64).all()


@pytest.mark.parametrize("kind", SATURATED)
def test_saturated_cases_hold_every_candidate_count(oracle, kind):
    """What keeps the test above honest (the oracle alone): the records hold one candidate (one list), two (two lists, PUs without bi-prediction) and three
    (with bi-prediction) - two-list controls give two and three, a two-list record never holds fewer than two."""
    seen, seen2 = set(), set()
    for ci, kw in enumerate(CONTROLS):
        p = default_params(192, 128, **kw)
        totals = set(np.unique(oracle_me(oracle, kind, 192, 128, p, key=ci)["pu"]["total"]).tolist())
        seen |= totals
        if p.num_lists == 2:
            seen2 |= totals
    assert seen == {1, 2, 3} and seen2 == {2, 3}


# ---- b. the smallest pictures a slot accepts ----

@pytest.mark.parametrize("ci", range(len(CONTROLS)))
@pytest.mark.parametrize("kind", ["motion", "x_binary"])
@pytest.mark.parametrize("w,h", [(64, 64), (72, 64), (64, 72), (136, 72)])
def test_me_matches_oracle_on_smallest_pictures(product, gpu_ctx, oracle, w, h, kind, ci):
    search_and_compare(product, gpu_ctx, oracle, kind, w, h, ci)


# ---- c. prep planes of saturated pictures ----

@pytest.mark.parametrize("w,h", [(72, 64), (328, 264)])
@pytest.mark.parametrize("kind", ["x_stripes", "x_binary"])
def test_prep_planes_of_saturated_pictures_match_oracle(product, gpu_ctx, oracle, kind, w, h):
    """The comparison of test_prep_planes_match_oracle on columns, rows and the one-sample checkerboard (t = 0, 1, 2 of x_stripes: the b, h and j filters
    leave the sample range at both ends) and on binary noise."""

    class Plane(C.Structure):
        _fields_ = [("data", C.c_void_p), ("stride", C.c_uint32), ("pad", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]

    frames, pics = clip(oracle, kind, w, h)
    for t, (luma, pic) in enumerate(zip(frames, pics)):
        upload(product, gpu_ctx, 0, luma)
        planes = (Plane * 6).from_address(pic.handle)
        for which, name in enumerate(["full", "quarter", "sixteenth", "hp_b", "hp_h", "hp_j"]):
            pl = planes[which]
            rows = pl.height + 2 * pl.pad
            want = np.ctypeslib.as_array((C.c_uint8 * (rows * pl.stride)).from_address(pl.data)).reshape(rows, pl.stride)
            got = read_plane(product, gpu_ctx, 0, which, w, h)
            assert got.shape == want.shape, (t, name)
            m = 0 if which < 3 else 2  # half-pel planes: the oracle leaves a 2-sample frame unwritten
            sl = (slice(m, rows - m), slice(m, pl.stride - m))
            assert np.array_equal(got[sl], want[sl]), "frame %d: plane %s differs" % (t, name)


# ---- d, e, f. batches whose jobs differ in size, controls and list count ----

TWO = dict(num_lists=2, temporal_layer_index=1)
MIXED = [  # clip, seed, width, height, ME controls, OIS controls
    ("motion", 7, 448, 328, dict(), OIS_VARIANTS[2]),
    ("x_whiteblack", SEED, 192, 128, dict(TWO, fractional_search_method=2, fractional_search_model=0, fractional_search_64x64=1, cu8x8_mode=0),
     OIS_VARIANTS[0]),
    ("x_binary", SEED, 64, 72, dict(TWO, search_area_width=21, search_area_height=13, enable_hme_level1=0, cu8x8_mode=0), OIS_VARIANTS[6]),
    ("noise", SEED, 328, 264, dict(search_area_width=75, search_area_height=70, temporal_layer_index=3), OIS_VARIANTS[5]),
    ("x_stripes", SEED, 136, 72, dict(TWO, enable_hme_flag=0, update_hme_search_center=0, fractional_search_model=2), OIS_VARIANTS[3]),
    ("motion", 13, 448, 328, dict(TWO, fractional_search_method=2), OIS_VARIANTS[4]),
]
assert OIS_VARIANTS[0].get("slice_is_intra") and OIS_VARIANTS[6].get("ois_kernel_level") and OIS_VARIANTS[5].get("limit_ois_to_dc_mode")
MIXED_SLOTS = 18

_mixed = {}


def teardown_module(module):
    if _mixed:
        _mixed["product"].svt_amd_context_destroy(_mixed["ctx"])
        _mixed.clear()


def mixed(product, oracle):
    """The context of the mixed batches: job i owns slots 3i (t = 0), 3i + 1 (t = 1, the searched picture) and 3i + 2 (t = 2).  Built once, with the oracle's
    records of every job alone."""
    if not _mixed:
        ctx = C.c_void_p()
        assert product.svt_amd_context_create(0, 448, 328, MIXED_SLOTS, C.byref(ctx)) == 0, product.svt_amd_last_error()
        _mixed.update(product=product, ctx=ctx, me_params=[], ois_params=[], frames=[], want_me=[], want_ois=[])
        for i, (kind, seed, w, h, kw, okw) in enumerate(MIXED):
            frames, _ = clip(oracle, kind, w, h, seed)
            for t in range(3):
                upload(product, ctx, 3 * i + t, frames[t])
            p, op = default_params(w, h, **kw), mk_params(w, h, **okw)
            want = oracle_me(oracle, kind, w, h, p, seed)
            _mixed["me_params"].append(p)
            _mixed["ois_params"].append(op)
            _mixed["frames"].append(frames[1])
            _mixed["want_me"].append(want)
            _mixed["want_ois"].append(S.oracle_ois_picture(oracle, op, frames[1], None if op.slice_is_intra else want))
    return _mixed


def me_jobs(m, order, edit=None):
    jobs = (S.MeJob * len(order))()
    for k, i in enumerate(order):
        jobs[k].params, jobs[k].cur_slot = m["me_params"][i], 3 * i + 1
        jobs[k].ref_slot[0], jobs[k].ref_slot[1] = 3 * i, 3 * i + 2
    if edit:
        edit(jobs)
    return jobs


def ois_jobs(m, order, edit=None):
    jobs = (S.OisJob * len(order))()
    for k, i in enumerate(order):
        jobs[k].params, jobs[k].cur_slot = m["ois_params"][i], 3 * i + 1
    if edit:
        edit(jobs)
    return jobs


def fetch_me(product, m):
    out = []
    for i, p in enumerate(m["me_params"]):
        got = np.zeros(S.lcu_count(p.luma_width, p.luma_height), S.ME_LCU_DTYPE)
        assert product.svt_amd_me_picture_fetch(m["ctx"], 3 * i + 1, got.ctypes.data) == 0, product.svt_amd_last_error()
        out.append(got)
    return out


def fetch_ois(product, m):
    out = []
    for i, p in enumerate(m["ois_params"]):
        got = np.zeros(S.lcu_count(p.luma_width, p.luma_height), S.OIS_LCU_DTYPE)
        assert product.svt_amd_ois_picture_fetch(m["ctx"], 3 * i + 1, got.ctypes.data) == 0, product.svt_amd_last_error()
        out.append(got)
    return out


def overwrite_me(product, m):
    """Other records into every job's slot (a one-list search of t = 1 in t = 2), so that records a launch leaves unwritten cannot pass for its result."""
    out = []
    for i, p in enumerate(m["me_params"]):
        out.append(me_picture(product, m["ctx"], default_params(p.luma_width, p.luma_height), 3 * i + 1, [3 * i + 2]))
        assert out[i].tobytes() != m["want_me"][i].tobytes()
    return out


def overwrite_ois(product, m):
    for i, p in enumerate(m["ois_params"]):
        other = mk_params(p.luma_width, p.luma_height, **OIS_VARIANTS[2 if p.slice_is_intra else 0])
        assert product.svt_amd_ois_picture_launch(m["ctx"], C.byref(other), 3 * i + 1) == 0, product.svt_amd_last_error()
    out = fetch_ois(product, m)
    for i in range(len(out)):
        assert not same(out[i], m["want_ois"][i])
    return out


def test_mixed_me_batch_matches_oracle_and_single_launches(product, oracle):
    m = mixed(product, oracle)
    ctx, params = m["ctx"], m["me_params"]
    alone = [me_picture(product, ctx, p, 3 * i + 1, [3 * i, 3 * i + 2]) for i, p in enumerate(params)]
    n = len(params)
    for order in (list(range(n)), list(range(n))[::-1]):  # the job with the most LCUs, the largest pool and two lists last, then first
        overwrite_me(product, m)
        assert product.svt_amd_me_batch_launch(ctx, me_jobs(m, order), n) == 0, product.svt_amd_last_error()
        for phase in (0, 1):  # the launcher asks for the largest pool over the jobs
            assert lds_bytes(product, None, phase) == max(lds_bytes(product, p, phase) for p in params), phase
        for i, got in enumerate(fetch_me(product, m)):
            what = "mixed batch, order %s, job %d" % (order, i)
            compare_all(got, m["want_me"][i], params[i], what)
            assert got.tobytes() == alone[i].tobytes(), what


def test_mixed_ois_batch_matches_oracle(product, oracle):
    """One OIS launch over the six pictures, six control sets, the ME records of the mixed batch left on the device."""
    m = mixed(product, oracle)
    n = len(m["ois_params"])
    overwrite_me(product, m)
    assert product.svt_amd_me_batch_launch(m["ctx"], me_jobs(m, range(n)), n) == 0, product.svt_amd_last_error()
    overwrite_ois(product, m)
    assert product.svt_amd_ois_batch_launch(m["ctx"], ois_jobs(m, range(n)), n) == 0, product.svt_amd_last_error()
    for i, got in enumerate(fetch_ois(product, m)):
        assert same(got, m["want_ois"][i]), "mixed OIS batch, job %d" % i


def test_refused_mixed_batch_queues_nothing(product, oracle):
    """A batch with one bad job is refused as a whole: the records of every slot stay what they were.  (They are overwritten with other records between the
    good batch and the refused ones: jobs that ran after all would put the good records back.)"""
    m = mixed(product, oracle)
    ctx, n = m["ctx"], len(m["me_params"])
    assert product.svt_amd_me_batch_launch(ctx, me_jobs(m, range(n)), n) == 0, product.svt_amd_last_error()
    assert product.svt_amd_ois_batch_launch(ctx, ois_jobs(m, range(n)), n) == 0, product.svt_amd_last_error()
    fetch_me(product, m), fetch_ois(product, m)
    overwrite_me(product, m)
    overwrite_ois(product, m)
    before_me = [g.tobytes() for g in fetch_me(product, m)]
    before_ois = [g.tobytes() for g in fetch_ois(product, m)]

    def bad_slot(jobs):
        jobs[5].cur_slot = MIXED_SLOTS

    def bad_width(jobs):
        jobs[2].params.luma_width += 8

    def bad_lists(jobs):
        jobs[4].params.num_lists = 3

    def bad_th_set(jobs):
        jobs[3].params.ois_th_set = 3

    for edit in (bad_slot, bad_width, bad_lists):
        assert product.svt_amd_me_batch_launch(ctx, me_jobs(m, range(n), edit), n) < 0, edit.__name__
        assert [g.tobytes() for g in fetch_me(product, m)] == before_me, edit.__name__
    assert product.svt_amd_ois_batch_launch(ctx, ois_jobs(m, range(n), bad_th_set), n) < 0
    assert [g.tobytes() for g in fetch_ois(product, m)] == before_ois
    assert [g.tobytes() for g in fetch_me(product, m)] == before_me
