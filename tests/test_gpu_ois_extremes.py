"""-m gpu: the open-loop intra search where the other GPU tests do not go.  Saturated pictures (every sample 0 or 255: SADs at the top of the 20-bit
distortion field, ME and DC SADs of 261,120 in GetOisPoint, both clips of the edge filters); x_islands, whose 32x32 islands no mode predicts better than
the reference's initial best, so that the search keeps the best mode and the SAD array of the CU before - the state the kernel decides without and then
replays serially; the same replay in the 35-column instance that a batch with an ois_kernel_level job runs for all of its jobs; the smallest pictures a slot
accepts; the compact records; the zero-motion SAD of saturated pictures.  Every comparison is bit-exact against the CPU oracle, on `candidate` and `total`
of every LCU; tests/golden/ois_x*.npz pin the oracle to the reference on the same clips and tests/test_ois_extremes_cpu.py shows what the inputs reach."""
import ctypes as C

import numpy as np
import pytest

import ois_extremes as X
import svtlib as S
from gpu_util import default_params, me_picture, upload
from test_gpu_ois import VARIANTS, mk_params, ois_picture, same

pytestmark = pytest.mark.gpu

SEED = 5
_own = {}


def teardown_module(module):
    if _own:
        _own["product"].svt_amd_context_destroy(_own["ctx"])
        _own.clear()


def search_on_device_records(product, ctx, oracle, kind, w, h, v, seed=SEED):
    """ME of frame 1 in frame 0 on the device, then the search twice: on the records where ME left them and on the same records through the host pointer"""
    f0, f1 = X.frame(kind, w, h, 0, seed), X.frame(kind, w, h, 1, seed)
    upload(product, ctx, 0, f0)
    upload(product, ctx, 1, f1)
    me = me_picture(product, ctx, default_params(w, h), 1, [0])
    p = mk_params(w, h, **VARIANTS[v])
    want = S.oracle_ois_picture(oracle, p, f1, None if p.slice_is_intra else me)
    assert same(ois_picture(product, ctx, p, 1, None), want), (kind, w, h, VARIANTS[v], "records on the device")
    assert same(ois_picture(product, ctx, p, 1, me), want), (kind, w, h, VARIANTS[v], "records through the host pointer")
    return me, want


# ---- a. saturated kinds ----

@pytest.mark.parametrize("v", range(len(VARIANTS)))
@pytest.mark.parametrize("kind", ["x_whiteblack", "x_binary", "x_stripes", "xc_blocks"])
def test_ois_matches_oracle_on_saturated_pictures(product, gpu_ctx, oracle, kind, v):
    me, want = search_on_device_records(product, gpu_ctx, oracle, kind, 192, 128, v)
    if kind == "x_whiteblack":  # white searched in black: every 32x32 ME SAD is 261,120
        assert (me["pu"]["distortion"][:, 1:5, 0] == X.SAT).all()


# ---- b. islands, seeded ME SADs ----

@pytest.mark.parametrize("layer", (0, 2, 3))
@pytest.mark.parametrize("th_set", (0, 1, 2))
def test_ois_matches_oracle_on_islands(product, gpu_ctx, oracle, th_set, layer):
    kind, w, h, seed = X.ISLANDS
    upload(product, gpu_ctx, 0, X.frame(kind, w, h, 1, seed))
    upload(product, gpu_ctx, 1, X.frame(kind, w, h, 3, seed))
    jobs = [j for j, kw in enumerate(X.ISLAND_JOBS) if kw["ois_th_set"] == th_set and kw["temporal_layer_index"] == layer]
    assert len(jobs) == 4
    carried = 0
    for j in jobs:
        luma, p, me, want, sat = X.island_job(oracle, j)
        got = ois_picture(product, gpu_ctx, p, j & 1, me)
        bad = np.nonzero((got["candidate"] != want["candidate"]).any(axis=(1, 2)) | (got["total"] != want["total"]).any(axis=1))[0]
        assert len(bad) == 0, (X.ISLAND_JOBS[j], "LCUs", bad.tolist(), "CUs 1..4 of the first: got",
                               [(int(c >> 24), int(c & 0xFFFFF)) for c in got["candidate"][bad[0], 1:5, 0]], got["total"][bad[0], 1:5].tolist(), "want",
                               [(int(c >> 24), int(c & 0xFFFFF)) for c in want["candidate"][bad[0], 1:5, 0]], want["total"][bad[0], 1:5].tolist())
        carried += int(X.carried(sat, want).sum())
    assert carried >= 8  # the path was taken


# ---- c. the 35-column instance ----

BATCH = [  # frame, controls
    (1, dict(ois_th_set=1, skip_ois_8x8=1, cu8x8_mode=1)),
    (3, dict(ois_th_set=2, temporal_layer_index=2, skip_ois_8x8=0, cu8x8_mode=0)),
    (1, dict(ois_th_set=0, temporal_layer_index=3, set_best_ois_distortion_to_valid=1, skip_ois_8x8=1, cu8x8_mode=1)),
    (3, dict(ois_kernel_level=1, skip_ois_8x8=1)),
    (1, dict(slice_is_intra=1)),
    (3, dict(limit_ois_to_dc_mode=1, skip_ois_8x8=1)),
]


def batch_context(product, oracle):
    """A context of its own: slots 0 and 1 hold the flat frames 0 and 2, slot 2 + i the picture of job i with its ME records (searched on the device in the
    flat frame before it) left in place.  Built once, with the oracle's records of every job."""
    if not _own:
        kind, w, h, seed = X.ISLANDS
        ctx = C.c_void_p()
        assert product.svt_amd_context_create(0, w, h, 2 + len(BATCH), C.byref(ctx)) == 0, product.svt_amd_last_error()
        _own.update(product=product, ctx=ctx, params=[], want=[], carried=[])
        upload(product, ctx, 0, X.frame(kind, w, h, 0, seed))
        upload(product, ctx, 1, X.frame(kind, w, h, 2, seed))
        for i, (t, kw) in enumerate(BATCH):
            upload(product, ctx, 2 + i, X.frame(kind, w, h, t, seed))
            p = mk_params(w, h, **kw)
            me = None if p.slice_is_intra else me_picture(product, ctx, default_params(w, h), 2 + i, [t // 2])
            want = S.oracle_ois_picture(oracle, p, X.frame(kind, w, h, t, seed), me)
            _own["params"].append(p)
            _own["want"].append(want)
            _own["carried"].append(int(X.carried(X.saturated(oracle, kind, w, h, t, seed), want).sum()) if i < 3 else 0)
    return _own


def fetch_all(product, m):
    out = []
    for i, p in enumerate(m["params"]):
        got = np.zeros(S.lcu_count(p.luma_width, p.luma_height), S.OIS_LCU_DTYPE)
        assert product.svt_amd_ois_picture_fetch(m["ctx"], 2 + i, got.ctypes.data) == 0, product.svt_amd_last_error()
        out.append(got)
    return out


def test_replay_in_the_35_column_instance(product, oracle):
    """One launch over island P pictures on the stage-1 path, one picture that ranks all modes, an I picture and a DC-only picture: the ranking job makes
    k_ois_picture<35> run every job, the carried CUs of the P pictures among them.  In both orders; every picture equals the oracle and its own launch."""
    m = batch_context(product, oracle)
    ctx, n = m["ctx"], len(BATCH)
    assert all(c >= 6 for c in m["carried"][:3]), m["carried"]
    alone = [ois_picture(product, ctx, p, 2 + i, None) for i, p in enumerate(m["params"])]
    for order in (list(range(n)), list(range(n))[::-1]):
        for i, p in enumerate(m["params"]):  # other records into every slot, so that records a launch leaves unwritten cannot pass for its result
            other = mk_params(p.luma_width, p.luma_height, **(dict(limit_ois_to_dc_mode=1, skip_ois_8x8=1) if i != 5 else dict(slice_is_intra=1)))
            assert product.svt_amd_ois_picture_launch(ctx, C.byref(other), 2 + i) == 0, product.svt_amd_last_error()
        for i, got in enumerate(fetch_all(product, m)):
            assert not same(got, m["want"][i]), i
        jobs = (S.OisJob * n)()
        for k, i in enumerate(order):
            jobs[k].params, jobs[k].cur_slot = m["params"][i], 2 + i
        assert product.svt_amd_ois_batch_launch(ctx, jobs, n) == 0, product.svt_amd_last_error()
        for i, got in enumerate(fetch_all(product, m)):
            assert same(got, m["want"][i]), ("against the oracle", order, i, BATCH[i])
            assert same(got, alone[i]), ("against its own launch", order, i, BATCH[i])


# ---- d. the smallest pictures a slot accepts ----

@pytest.mark.parametrize("v", range(len(VARIANTS)))
@pytest.mark.parametrize("kind", ["motion", "x_binary"])
@pytest.mark.parametrize("w,h", [(64, 64), (72, 64), (64, 72), (136, 72)])
def test_ois_matches_oracle_on_smallest_pictures(product, gpu_ctx, oracle, w, h, kind, v):
    search_on_device_records(product, gpu_ctx, oracle, kind, w, h, v)


# ---- e. compact records ----

def test_compact_records_of_an_island_picture(product, gpu_ctx, oracle):
    luma, p, me, want, sat = X.island_job(oracle, 20)
    assert X.carried(sat, want).any()
    upload(product, gpu_ctx, 0, luma)
    full = ois_picture(product, gpu_ctx, p, 0, me)
    assert same(full, want)
    n = len(full)
    for nc in (7, 9, 18):
        compact = np.zeros(n, np.dtype([("candidate", "<u4", (S.ME_PU_COUNT, nc)), ("total", "u1", (S.ME_PU_COUNT,)), ("pad", "u1", (3,))]))
        assert compact.dtype.itemsize == S.ME_PU_COUNT * nc * 4 + 88
        compact["total"] = 0xEE
        assert product.svt_amd_ois_picture_fetch_compact_async(gpu_ctx, 0, nc, compact.ctypes.data) == 0, product.svt_amd_last_error()
        assert product.svt_amd_synchronize(gpu_ctx) == 0, product.svt_amd_last_error()
        assert np.array_equal(compact["candidate"], full["candidate"][:, :, :nc]), nc
        assert np.array_equal(compact["total"], full["total"]), nc


# ---- f. zero-motion SAD of saturated pictures ----

@pytest.mark.parametrize("kind,t,w,h", [("x_whiteblack", 1, 192, 128), ("x_whiteblack", 2, 192, 128), ("x_whiteblack", 3, 200, 136), ("x_stripes", 1, 192, 128),
                                        ("x_stripes", 2, 200, 136)])
def test_zz_sad_matches_oracle_on_saturated_pictures(product, gpu_ctx, oracle, kind, t, w, h):
    """Frame t against frame t - 1 through svt_amd_zz_sad_picture; white against black, every sample of the 1/16 planes differs by 255."""
    cur, prev = X.frame(kind, w, h, t, SEED), X.frame(kind, w, h, t - 1, SEED)
    upload(product, gpu_ctx, 0, prev)
    upload(product, gpu_ctx, 1, cur)
    got = np.zeros(S.lcu_count(w, h), X.ZZ_DTYPE)
    product.svt_amd_zz_sad_picture.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert product.svt_amd_zz_sad_picture(gpu_ctx, 1, 0, got.ctypes.data) == 0, product.svt_amd_last_error()
    assert np.array_equal(got, X.oracle_zz(oracle, cur, prev))
    if kind == "x_whiteblack" and t == 1:
        assert (got["sad"] == 16 * 16 * 255).all()
