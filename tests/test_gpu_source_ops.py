"""The batched source-based operations on the device (include/svt_hevc_amd.h "Batched source-based operations"; svt-hevc_amd/csrc/sbo_kernels.hip) through the
C-ABI: svt_amd_source_ops_batch_launch against the records the REFERENCE's own functions left for the seeded inputs (tests/golden/sbo_*.npz), against the
restatement (tests/sbo_numpy.py, pinned on the same files by tests/test_sbo_cpu.py) on further seeded records, and chained on one lane behind ME, OIS and the
three picture-analysis batches with nothing downloaded in between.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import pa_detect_numpy as PN
import pa_detect_pictures as P
import sbo_numpy as N
import sbo_records as R
import sidelib as L
import svtlib as S
from gpu_util import default_params, upload
from pa_batch_util import DeviceBuffer, is_sentinel, make_context, ok, refused, round_up as _up
from test_sbo_cpu import CASES, load_case

pytestmark = pytest.mark.gpu
RECORDS = ("stats", "ref_stats", "chroma", "detect", "histogram", "me", "ois")


@pytest.fixture(scope="module")
def lib(product):
    return R.declare(PN.declare(L.declare(product)))


class Pictures:
    """the records of a list of pictures in device memory, and the jobs that point at them"""

    def __init__(self, lib, ctx, w, h, rw, rh, recs, jobs):
        self.lib, self.ctx, self.w, self.h, self.rw, self.rh, self.recs, self.jobs = lib, ctx, w, h, rw, rh, recs, jobs
        self.nl = S.lcu_count(w, h)
        self.keep, self.at = [], []
        size = sum(_up(r[k].nbytes) for r in recs for k in RECORDS) + sum(_up(z.nbytes) for r in recs for z in r["zz"])
        self.dev = DeviceBuffer(lib, ctx, max(size, 256))
        off = 0
        for r in recs:
            at = {}
            for k in RECORDS:
                at[k], off = off, self._put(r[k], off)
            at["zz"] = []
            for z in r["zz"]:
                at["zz"].append(off)
                off = self._put(z, off)
            self.at.append(at)

    def _put(self, a, off):
        a = np.ascontiguousarray(a)
        self.keep.append(a)
        self.dev.put(a, off)
        return off + _up(a.nbytes)

    def job(self, i, slot_records=None):
        """slot_records: (cur_slot, me from the slot, ois from the slot) or None - both tables given"""
        j, jb, at = R.SboJob(), self.jobs[i], self.at[i]
        j.stats, j.chroma, j.detect, j.histogram = (self.dev.at(at[k]) for k in ("stats", "chroma", "detect", "histogram"))
        j.ref_stats = self.dev.at(at["ref_stats"]) if jb["slice_type"] != 0 else None
        for k, o in enumerate(at["zz"]):
            j.zz[k] = self.dev.at(o)
        j.me, j.ois, j.cur_slot = self.dev.at(at["me"]), self.dev.at(at["ois"]), -1
        if slot_records:
            j.cur_slot = slot_records[0]
            j.me, j.ois = (None if slot_records[1] else j.me), (None if slot_records[2] else j.ois)
        j.zz_count, j.slice_type, j.temporal_layer_index, j.is_used_as_reference = jb["zz_count"], jb["slice_type"], jb["layer"], jb["ref"]
        j.resolution_class, j.skip_ois_8x8, j.cu8x8_mode, j.want_qpm = jb["cls"], jb["skip"], jb["cu8"], jb["qpm"]
        return j

    def job_array(self, order):
        jobs = (R.SboJob * len(order))()
        for k, i in enumerate(order):
            jobs[k] = self.job(i)
        return jobs

    def free(self):
        self.dev.free()


class Results:
    """the two output arrays of an n-picture batch, filled with SENTINEL"""

    def __init__(self, lib, ctx, n, w, h):
        self.lib, self.n, self.nl = lib, n, S.lcu_count(w, h)
        self.lcu, self.pic = DeviceBuffer(lib, ctx, n * self.nl * R.SBO_LCU_DTYPE.itemsize), DeviceBuffer(lib, ctx, n * R.SBO_PIC_DTYPE.itemsize)

    def table(self):
        return R.SboArrays(self.lcu.ptr.value, self.pic.ptr.value)

    def download(self):
        return self.lcu.get().view(R.SBO_LCU_DTYPE).reshape(self.n, self.nl), self.pic.get().view(R.SBO_PIC_DTYPE)

    def untouched(self):
        return is_sentinel(self.lcu.get()) and is_sentinel(self.pic.get())

    def free(self):
        self.lcu.free(), self.pic.free()


def launch(lib, ctx, jobs, n, w, h, rw, rh, table):
    return lib.svt_amd_source_ops_batch_launch(ctx, jobs, n, w, h, rw, rh, C.byref(table))


def run(lib, ctx, pics, order):
    """one batch of the pictures `order` -> (lcu [n][lcus], picture [n])"""
    out = Results(lib, ctx, len(order), pics.w, pics.h)
    t = out.table()
    ok(lib, launch(lib, ctx, pics.job_array(order), len(order), pics.w, pics.h, pics.rw, pics.rh, t))
    got = out.download()
    out.free()
    return got


def same(got_lcu, got_pic, want_lcu, want_pic, what):
    for f in R.LCU_FIELDS:
        assert np.array_equal(got_lcu[f], want_lcu[f]), (what, f, np.flatnonzero(got_lcu[f] != want_lcu[f])[:6].tolist())
    for f in R.PIC_FIELDS:
        assert np.array_equal(got_pic[f], want_pic[f]), (what, f, got_pic[f], want_pic[f])
    assert not got_lcu["pad"].any() and not got_pic["pad"].any(), (what, "pad bytes")


def restate(w, h, rec, jb):
    lcu, pic, _ = N.source_ops(w, h, rec if jb["slice_type"] != 0 else dict(rec, ref_stats=None), jb)
    return lcu, pic


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_fixture_gives_what_the_reference_computed(lib, name):
    w, h, rw, rh, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = Pictures(lib, ctx, w, h, rw, rh, R.case_inputs(name), jobs)
    try:
        for first in range(0, len(jobs), 6):                      # batches of at most 6
            order = list(range(first, min(first + 6, len(jobs))))
            lcu, pic = run(lib, ctx, pics, order)
            for k, i in enumerate(order):
                same(lcu[k], pic[k], g["lcu"][i], g["picture"][i], (name, i))
    finally:
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 2. further seeded records against the restatement; a mixed batch in both orders ------------------------------------------------------------

VARIANT_JOBS = [R.job(R.I, 0, 1, 2, qpm=1, hist="dark"), R.job(R.P, 0, 1, 17, qpm=1, skip=1, activity="active", hist="wrap"),
                R.job(R.B, 1, 0, 3, qpm=1, cu8=1, activity="moderate", hist="dark_light"), R.job(R.B, 5, 1, 0, cls=2), R.job(R.B, 3, 1, 17, cls=3, activity="active"),
                R.job(R.P, 2, 0, 1, hist="dark_no_white")]


@pytest.mark.parametrize("w,h,rw,rh,seed", [(48, 40, 1, 1, 23), (200, 136, 3, 3, 29), (960, 128, 8, 2, 31), (1088, 576, 4, 4, 37)])
def test_seeded_variants_match_the_restatement(lib, w, h, rw, rh, seed):
    """no complete LCU at all; partial column and row in a 4 x 3 picture; two LCU rows (no interior); 17 x 9 LCUs, more than one LDS stride of the finish kernel's
    QPM partials"""
    recs = [R.make_inputs(w, h, rw, rh, seed, i, jb) for i, jb in enumerate(VARIANT_JOBS)]
    ctx = make_context(lib, max(w, 64), max(h, 64), 1)
    pics = Pictures(lib, ctx, w, h, rw, rh, recs, VARIANT_JOBS)
    try:
        lcu, pic = run(lib, ctx, pics, list(range(6)))
        for i, (jb, rec) in enumerate(zip(VARIANT_JOBS, recs)):
            same(lcu[i], pic[i], *restate(w, h, rec, jb), what=(w, h, i))
        if w == 48:
            assert not pic["complete_lcu_count"].any() and not pic["non_moving_index_average"].any()
    finally:
        pics.free()
        lib.svt_amd_context_destroy(ctx)


def test_a_mixed_batch_in_both_orders_equals_the_single_launches(lib):
    name = "plain_320x256"
    w, h, rw, rh, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = Pictures(lib, ctx, w, h, rw, rh, R.case_inputs(name), jobs)
    mixed = [0, 2, 4, 5, 6, 8]                                   # I / P / B, layers 0..2, windows of 0, 1 and 17, want_qpm both ways
    try:
        single = [run(lib, ctx, pics, [i]) for i in mixed]
        for order in (mixed, mixed[::-1]):
            lcu, pic = run(lib, ctx, pics, order)
            for k, i in enumerate(order):
                s_lcu, s_pic = single[mixed.index(i)]
                assert lcu[k].tobytes() == s_lcu[0].tobytes() and pic[k].tobytes() == s_pic[0].tobytes(), (order, i)
                same(lcu[k], pic[k], g["lcu"][i], g["picture"][i], (order, i))
    finally:
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 3. the chain on one lane, real planes ---------------------------------------------------------------------------------------------------------

def test_chain_on_one_lane_reads_the_records_where_they_lie(lib):
    """upload, ME, OIS, side statistics, chroma statistics, detectors and the source-based operations (ME / OIS records of the slot: me = ois = NULL) queued on
    one lane with nothing downloaded in between; afterwards the intermediate records are downloaded and fed to the restatement"""
    w, h, rw, rh, seed = 320, 256, 4, 4, 41
    nl, plane = S.lcu_count(w, h), (w // 2) * (h // 2)
    ctx = make_context(lib, w, h, 4)
    frames = [P.gen_luma("motion", w, h, t, seed) for t in range(4)]
    cb, cr = (np.ascontiguousarray(a) for a in P.gen_chroma("motion", w, h, 1, seed))
    jb = R.job(R.B, 0, 1, 3, qpm=1)
    sizes = L.numpy_sizes(w, h, rw, rh)
    buf = dict(stats=DeviceBuffer(lib, ctx, 3 * sizes[L.BLOCK_STATS]), zz=DeviceBuffer(lib, ctx, 3 * sizes[L.ZZ_SAD]), hist=DeviceBuffer(lib, ctx, 3 * sizes[L.HISTOGRAM]),
               planes=DeviceBuffer(lib, ctx, 2 * plane), means=DeviceBuffer(lib, ctx, nl * 48), dlcu=DeviceBuffer(lib, ctx, nl * 48), dpic=DeviceBuffer(lib, ctx, 8))
    out = Results(lib, ctx, 1, w, h)
    try:
        for s, f in enumerate(frames):
            upload(lib, ctx, s, f)
        buf["planes"].put(cb, 0), buf["planes"].put(cr, plane)
        mj, oj = (S.MeJob * 1)(), (S.OisJob * 1)()
        mj[0].params, mj[0].cur_slot = default_params(w, h, num_lists=2, temporal_layer_index=0, cu8x8_mode=0), 1
        mj[0].ref_slot[0], mj[0].ref_slot[1] = 0, 2
        op = S.OisParams()
        op.luma_width, op.luma_height, op.ois_th_set, op.temporal_layer_index = w, h, 1, 0
        oj[0].params, oj[0].cur_slot = op, 1
        ok(lib, lib.svt_amd_me_batch_launch(ctx, mj, 1))
        ok(lib, lib.svt_amd_ois_batch_launch(ctx, oj, 1))
        # pictures 1, 2, 3 of the window: block statistics and histograms of each, the zz records of each against the picture in front of it
        side = L.make_jobs([(1, 0, 1, 0, 1), (2, 1, 1, 0, 1), (3, 2, 1, 0, 1)])
        st = L.SideArrays(block_stats=buf["stats"].ptr.value, zz=buf["zz"].ptr.value, histogram=buf["hist"].ptr.value)
        ok(lib, lib.svt_amd_side_stats_batch_launch(ctx, side, 3, rw, rh, C.byref(st)))
        cj = (PN.ChromaJob * 1)()
        cj[0].cb, cj[0].cr, cj[0].pitch, cj[0].want_means, cj[0].want_histogram = buf["planes"].at(0), buf["planes"].at(plane), w // 2, 1, 0
        ct = PN.ChromaArrays(buf["means"].ptr.value, None, None, None)
        ok(lib, lib.svt_amd_chroma_stats_batch_launch(ctx, cj, 1, w, h, rw, rh, C.byref(ct)))
        dj = (PN.DetectJob * 1)()
        dj[0].stats, dj[0].chroma, dj[0].want_edge16, dj[0].resolution_class = buf["stats"].at(0), buf["means"].at(0), 1, 0
        dt = PN.DetectArrays(buf["dlcu"].ptr.value, buf["dpic"].ptr.value)
        ok(lib, lib.svt_amd_picture_detect_batch_launch(ctx, dj, 1, w, h, C.byref(dt)))
        j = (R.SboJob * 1)()
        j[0].stats, j[0].ref_stats, j[0].chroma, j[0].detect, j[0].histogram = buf["stats"].at(0), buf["stats"].at(sizes[L.BLOCK_STATS]), buf["means"].at(0), buf["dlcu"].at(0), buf["hist"].at(0)
        for k in range(3):
            j[0].zz[k] = buf["zz"].at(k * sizes[L.ZZ_SAD])
        j[0].me, j[0].ois, j[0].cur_slot = None, None, 1
        j[0].zz_count, j[0].slice_type, j[0].temporal_layer_index, j[0].is_used_as_reference, j[0].want_qpm = 3, jb["slice_type"], jb["layer"], jb["ref"], jb["qpm"]
        t = out.table()
        ok(lib, launch(lib, ctx, j, 1, w, h, rw, rh, t))
        lcu, pic = out.download()                                   # the first wait of the chain
        me, ois = np.zeros(nl, S.ME_LCU_DTYPE), np.zeros(nl, S.OIS_LCU_DTYPE)
        ok(lib, lib.svt_amd_me_picture_fetch(ctx, 1, me.ctypes.data))
        ok(lib, lib.svt_amd_ois_picture_fetch(ctx, 1, ois.ctypes.data))
        stats = buf["stats"].get().view(S.PA_LCU_STATS_DTYPE).reshape(3, nl)
        rec = dict(stats=stats[0], ref_stats=stats[1], chroma=buf["means"].get().view(PN.LCU_CHROMA_DTYPE), detect=buf["dlcu"].get().view(PN.LCU_DETECT_DTYPE),
                   histogram=buf["hist"].get().view(np.uint32).reshape(3, rw, rh, 256)[0], zz=buf["zz"].get().view(L.ZZ_DTYPE).reshape(3, nl), me=me, ois=ois)
        assert me["pu"]["distortion"][:, 0, 0].any() and (ois["candidate"][:, 1, 0] & 0xFFFFF).any()
        same(lcu[0], pic[0], *restate(w, h, rec, jb), what="chain")
    finally:
        out.free()
        for b in buf.values():
            b.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 4. two batches back to back --------------------------------------------------------------------------------------------------------------------

def test_two_batches_back_to_back_on_one_lane(lib):
    """the second batch is queued while the first may still run: it reuses the descriptor table and the scratch (QPM partials, flag bytes) of the first"""
    name = "partial_416x240"
    w, h, rw, rh, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = Pictures(lib, ctx, w, h, rw, rh, R.case_inputs(name), jobs)
    orders = ([0, 1, 2, 3, 4, 5], [8, 7, 6, 5, 3, 1])
    outs = [Results(lib, ctx, 6, w, h) for _ in orders]
    try:
        for order, out in zip(orders, outs):
            t = out.table()
            ok(lib, launch(lib, ctx, pics.job_array(order), 6, w, h, rw, rh, t))
        for order, out in zip(orders, outs):
            lcu, pic = out.download()
            for k, i in enumerate(order):
                same(lcu[k], pic[k], g["lcu"][i], g["picture"][i], (order, i))
    finally:
        for out in outs:
            out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_entry_and_queue_nothing(lib):
    name = "plain_320x256"
    w, h, rw, rh, seed, jobs = R.CASES[name]
    ctx = make_context(lib, w, h, 3)
    pics = Pictures(lib, ctx, w, h, rw, rh, R.case_inputs(name), jobs)
    out = Results(lib, ctx, 2, w, h)
    t = out.table()
    upload(lib, ctx, 0, S.gen_luma("motion", w, h, 0, 5))          # slot 0: a picture of the batch's size, but no ME / OIS records
    upload(lib, ctx, 1, S.gen_luma("motion", 256, 192, 0, 5))      # slot 1: a picture of another size; slot 2: no picture

    def bad(change, i=2, slot_records=None, what=None, **launch_args):
        pair = (R.SboJob * 2)()
        pair[0], pair[1] = pics.job(0), pics.job(i, slot_records)
        change(pair[1])
        args = dict(n=2, w=w, h=h, rw=rw, rh=rh, table=t)
        args.update(launch_args)
        refused(lib, launch(lib, ctx, pair, args["n"], args["w"], args["h"], args["rw"], args["rh"], args["table"]), R.ENTRY, what)
        assert b"job 1" in lib.svt_amd_last_error() or launch_args, lib.svt_amd_last_error()

    try:
        for field in ("stats", "chroma", "detect", "histogram"):
            bad(lambda j: setattr(j, field, None), what=field)
        bad(lambda j: setattr(j, "zz_count", 18), what="zz_count")
        bad(lambda j: j.zz.__setitem__(0, None), what="zz[0]")
        bad(lambda j: setattr(j, "temporal_layer_index", 6), what="layer")
        bad(lambda j: setattr(j, "resolution_class", 4), what="class")
        bad(lambda j: setattr(j, "slice_type", 3), what="slice type")
        bad(lambda j: setattr(j, "me", None), i=2, what="P picture without ME")               # cur_slot -1
        bad(lambda j: setattr(j, "ois", None), i=2, what="P picture without OIS")
        bad(lambda j: setattr(j, "me", None), i=0, what="want_qpm without ME")
        bad(lambda j: None, i=4, slot_records=(0, 1, 0), what="incomplete ME records")
        bad(lambda j: None, i=4, slot_records=(0, 0, 1), what="incomplete OIS records")
        bad(lambda j: None, i=4, slot_records=(1, 1, 1), what="a slot of another size")
        bad(lambda j: None, i=4, slot_records=(2, 1, 1), what="a slot without a picture")
        bad(lambda j: None, i=4, slot_records=(3, 1, 1), what="no such slot")
        bad(lambda j: None, what="too many LCUs", w=8256, h=8256)
        bad(lambda j: None, what="larger than the context", w=w + 64)
        bad(lambda j: None, what="regions", rw=9, rh=8)
        bad(lambda j: None, what="no lcu array", table=R.SboArrays(None, out.pic.ptr.value))
        bad(lambda j: None, what="no picture array", table=R.SboArrays(out.lcu.ptr.value, None))
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert out.untouched()
        # an I picture without want_qpm reads neither table nor the slot
        j = (R.SboJob * 1)()
        j[0] = pics.job(0)
        j[0].want_qpm, j[0].me, j[0].ois, j[0].cur_slot = 0, None, None, -5
        ok(lib, launch(lib, ctx, j, 1, w, h, rw, rh, t))
        lcu, pic = out.download()
        want_lcu, want_pic = restate(w, h, pics.recs[0], dict(jobs[0], qpm=0))
        same(lcu[0], pic[0], want_lcu, want_pic, "I picture without records")
        assert is_sentinel(lcu[1]) and is_sentinel(pic[1:])
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 6. a batch of one and the bounds of the job count ------------------------------------------------------------------------------------------------

def test_a_batch_of_one_and_the_header_bounds(lib):
    name = "one_64x64"
    w, h, rw, rh, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = Pictures(lib, ctx, w, h, rw, rh, R.case_inputs(name), jobs)
    out = Results(lib, ctx, 256, w, h)
    t = out.table()
    try:
        for n in (0, -1, 257):
            refused(lib, launch(lib, ctx, pics.job_array([3]), n, w, h, rw, rh, t), R.ENTRY, n)
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert out.untouched()
        lcu, pic = run(lib, ctx, pics, [5])
        same(lcu[0], pic[0], g["lcu"][5], g["picture"][5], "a batch of one")
        order = [i % len(jobs) for i in range(256)]                # the largest batch
        ok(lib, launch(lib, ctx, pics.job_array(order), 256, w, h, rw, rh, t))
        lcu, pic = out.download()
        for k in (0, 1, 127, 254, 255):
            same(lcu[k], pic[k], g["lcu"][order[k]], g["picture"][order[k]], ("256", k))
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)
