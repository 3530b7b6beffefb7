"""The batched mode-decision configuration on the device (include/svt_hevc_amd.h "Batched mode-decision configuration"; svt-hevc_amd/csrc/mdc_kernels.hip)
through the C-ABI: svt_amd_md_config_batch_launch against the records the REFERENCE's own functions left for the seeded inputs (tests/golden/mdc_*.npz),
against the restatement (tests/mdc_numpy.py, pinned on the same files by tests/test_mdc_cpu.py) on further seeded records at the shapes where the kernels take
another path, and chained on one lane behind ME, OIS and the source-based operations with the ME records read where they lie.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import mdc_numpy as N
import mdc_records as R
import mdclib as M
import pa_detect_numpy as PN
import pa_detect_pictures as P
import sbo_records as SR
import sidelib as L
import svtlib as S
from gpu_util import default_params, upload
from pa_batch_util import DeviceBuffer, is_sentinel, make_context, markers, ok, refused, round_up as _up
from test_mdc_cpu import CASES, load_case, tables

pytestmark = pytest.mark.gpu
RECORDS = ("me", "stats", "detect", "sbo_lcu", "sbo_pic", "pic_detect", "noise_pic")
LAMBDA, SPLIT_BITS = 261, [12171, 78934]        # for the seeded variants: any SAD lambda and pair of split-flag rates; the restatement takes the same


@pytest.fixture(scope="module")
def lib(product):
    return M.declare(product)


class Pictures:
    """the records of a list of pictures in device memory, and the jobs that point at them.  tabs: (lambda, split bits) per picture"""

    def __init__(self, lib, ctx, w, h, recs, jobs, tabs):
        self.lib, self.ctx, self.w, self.h, self.recs, self.jobs, self.tabs = lib, ctx, w, h, recs, jobs, tabs
        self.keep, self.at = [], []
        size = sum(_up(r[k].nbytes) for r in recs for k in RECORDS) + sum(_up(r["stationary_edge"].nbytes) for r in recs if r["stationary_edge"] is not None)
        self.dev = DeviceBuffer(lib, ctx, max(size, 256))
        off = 0
        for r in recs:
            at = {}
            for k in RECORDS:
                at[k], off = off, self._put(r[k], off)
            if r["stationary_edge"] is not None:
                at["stationary_edge"], off = off, self._put(r["stationary_edge"], off)
            self.at.append(at)

    def _put(self, a, off):
        a = np.ascontiguousarray(a)
        self.keep.append(a)
        self.dev.put(a, off)
        return off + _up(a.nbytes)

    def job(self, i):
        j, at = M.MdcJob(), self.at[i]
        for k in RECORDS:
            setattr(j, k, self.dev.at(at[k]))
        j.stationary_edge = self.dev.at(at["stationary_edge"]) if "stationary_edge" in at else None
        j.cur_slot = -1
        return M.fill_scalars(j, self.jobs[i], *self.tabs[i])

    def job_array(self, order):
        jobs = (M.MdcJob * len(order))()
        for k, i in enumerate(order):
            jobs[k] = self.job(i)
        return jobs

    def free(self):
        self.dev.free()


class Results:
    """the two output arrays of an n-picture batch, filled with SENTINEL"""

    def __init__(self, lib, ctx, n, w, h):
        self.lib, self.n, self.nl = lib, n, S.lcu_count(w, h)
        self.lcu, self.pic = DeviceBuffer(lib, ctx, n * self.nl * R.MDC_LCU_DTYPE.itemsize), DeviceBuffer(lib, ctx, n * R.MDC_PIC_DTYPE.itemsize)

    def table(self):
        return M.MdcArrays(self.lcu.ptr.value, self.pic.ptr.value)

    def download(self):
        return self.lcu.get().view(R.MDC_LCU_DTYPE).reshape(self.n, self.nl), self.pic.get().view(R.MDC_PIC_DTYPE)

    def untouched(self):
        return is_sentinel(self.lcu.get()) and is_sentinel(self.pic.get())

    def free(self):
        self.lcu.free(), self.pic.free()


def launch(lib, ctx, jobs, n, w, h, table):
    return lib.svt_amd_md_config_batch_launch(ctx, jobs, n, w, h, C.byref(table))


def run(lib, ctx, pics, order):
    """one batch of the pictures `order` -> (lcu [n][lcus], picture [n])"""
    out = Results(lib, ctx, len(order), pics.w, pics.h)
    t = out.table()
    ok(lib, launch(lib, ctx, pics.job_array(order), len(order), pics.w, pics.h, t))
    got = out.download()
    out.free()
    return got


def same(got_lcu, got_pic, want_lcu, want_pic, what):
    for f in R.LCU_FIELDS:
        assert np.array_equal(got_lcu[f], want_lcu[f]), (what, f, np.flatnonzero((got_lcu[f] != want_lcu[f]).reshape(got_lcu.size, -1).any(1))[:6].tolist())
    for f in R.PIC_FIELDS:
        assert np.array_equal(got_pic[f], want_pic[f]), (what, f, got_pic[f], want_pic[f])
    assert not got_lcu["pad"].any() and not got_lcu["pad0"].any() and not got_pic["pad"].any() and not got_pic["pad0"].any(), (what, "pad bytes")


def fixture_pictures(lib, ctx, name):
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    return g, Pictures(lib, ctx, w, h, R.case_inputs(name), jobs, [tables(g, j) for j in range(len(jobs))])


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_fixture_gives_what_the_reference_computed(lib, name):
    w, h, seed, jobs = R.CASES[name]
    ctx = make_context(lib, w, h, 1)
    g, pics = fixture_pictures(lib, ctx, name)
    try:
        lcu, pic = run(lib, ctx, pics, list(range(len(jobs))))        # one batch of all the case's pictures
        for i in range(len(jobs)):
            same(lcu[i], pic[i], g["lcu"][i], g["picture"][i], (name, i))
    finally:
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 2. further seeded records against the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,seed", [(48, 40, 43), (128, 64, 47), (192, 128, 53), (960, 136, 59), (2112, 1152, 61)])
def test_seeded_variants_match_the_restatement(lib, w, h, seed):
    """one partial LCU; two LCUs and no aura candidate; a 3 x 2 grid whose only aura candidate (top row, centre) is an edge LCU; a partial bottom row; 594 LCUs -
    more than one LCU a thread in the budget kernel.  The usual jobs: every depth mode, stationary-edge bytes set and NULL"""
    jobs = R._usual_jobs(cls=3 if w == 2112 else 2 if w == 960 else 0)
    assert {jb["stationary"] for jb in jobs} == {"none", "some"} and {jb["depth_mode"] for jb in jobs} == {0, 1, 2, 3}
    recs = [R.make_inputs(w, h, seed, i, jb) for i, jb in enumerate(jobs)]
    ctx = make_context(lib, max(w, 64), max(h, 64), 1)
    pics = Pictures(lib, ctx, w, h, recs, jobs, [(LAMBDA + 37 * i, SPLIT_BITS) for i in range(len(jobs))])
    try:
        lcu, pic = run(lib, ctx, pics, list(range(len(jobs))))
        for i, (jb, rec) in enumerate(zip(jobs, recs)):
            want_lcu, want_pic, _ = N.md_config(w, h, rec, jb, *pics.tabs[i])
            same(lcu[i], pic[i], want_lcu, want_pic, (w, h, i))
    finally:
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 3. a mixed batch in both orders ---------------------------------------------------------------------------------------------------------------

def test_a_mixed_batch_in_both_orders_equals_the_single_launches(lib):
    name = "partial_416x240"
    w, h, seed, jobs = R.CASES[name]
    ctx = make_context(lib, w, h, 1)
    g, pics = fixture_pictures(lib, ctx, name)
    mixed = [0, 1, 3, 4, 9, 10, 11]                              # P / B, layers 0..3, stationary bytes set and NULL, LCU switch, full 85, full 84 and BDP pictures
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


# ---- 4. two batches back to back --------------------------------------------------------------------------------------------------------------------

def test_two_batches_back_to_back_on_one_lane(lib):
    """the second batch is queued while the first may still run: it reuses the descriptor table and the scratch (scores, flags) of the first - stored into,
    never accumulated"""
    name = "many_704x640"
    w, h, seed, jobs = R.CASES[name]
    ctx = make_context(lib, w, h, 1)
    g, pics = fixture_pictures(lib, ctx, name)
    orders = ([0, 1, 2, 3, 4, 5], [11, 8, 7, 6, 5, 1])
    outs = [Results(lib, ctx, 6, w, h) for _ in orders]
    try:
        for order, out in zip(orders, outs):
            t = out.table()
            ok(lib, launch(lib, ctx, pics.job_array(order), 6, w, h, t))
        for order, out in zip(orders, outs):
            lcu, pic = out.download()
            for k, i in enumerate(order):
                same(lcu[k], pic[k], g["lcu"][i], g["picture"][i], (order, i))
    finally:
        for out in outs:
            out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 5. the chain on one lane -------------------------------------------------------------------------------------------------------------------------

def test_chain_on_one_lane_reads_the_slots_me_records(lib):
    """upload, ME, OIS, source-based operations (their LCU and picture records feed this entry where they lie) and this entry with me = NULL, queued on one lane
    with nothing downloaded in between.  The result equals the run with the ME records given by pointer and the restatement on the downloaded records, and the
    call waits as often as the source-ops consumer in front of it did"""
    w, h, seed = 320, 256, 67
    nl = S.lcu_count(w, h)
    SR.declare(PN.declare(L.declare(lib)))
    ctx = make_context(lib, w, h, 3)
    jb = R.job(R.B, 0, 1, 8, 2, qp=30, noise=3, stationary="some")
    rec = R.make_inputs(w, h, seed, 0, jb)
    srec = SR.make_inputs(w, h, 4, 4, seed, 0, SR.job(SR.B, 0, 1, 3, qpm=1))
    side = ("stats", "ref_stats", "chroma", "detect", "histogram")
    size = sum(_up(srec[k].nbytes) for k in side) + sum(_up(z.nbytes) for z in srec["zz"]) + sum(_up(rec[k].nbytes) for k in ("pic_detect", "noise_pic", "stationary_edge"))
    dev, keep, at, off = DeviceBuffer(lib, ctx, size), [], {}, 0

    def put(a):
        nonlocal off
        a = np.ascontiguousarray(a)
        keep.append(a)
        dev.put(a, off)
        where, off = dev.at(off), off + _up(a.nbytes)
        return where

    sbo_lcu, sbo_pic = DeviceBuffer(lib, ctx, nl * SR.SBO_LCU_DTYPE.itemsize), DeviceBuffer(lib, ctx, SR.SBO_PIC_DTYPE.itemsize)
    me_dev = DeviceBuffer(lib, ctx, nl * S.ME_LCU_DTYPE.itemsize)
    outs = [Results(lib, ctx, 1, w, h) for _ in range(2)]
    try:
        for s in range(3):
            upload(lib, ctx, s, P.gen_luma("motion", w, h, s, seed))
        mj, oj = (S.MeJob * 1)(), (S.OisJob * 1)()
        mj[0].params, mj[0].cur_slot = default_params(w, h, num_lists=2, temporal_layer_index=0, cu8x8_mode=0), 1
        mj[0].ref_slot[0], mj[0].ref_slot[1] = 0, 2
        op = S.OisParams()
        op.luma_width, op.luma_height, op.ois_th_set, op.temporal_layer_index = w, h, 1, 0
        oj[0].params, oj[0].cur_slot = op, 1
        ok(lib, lib.svt_amd_me_batch_launch(ctx, mj, 1))
        ok(lib, lib.svt_amd_ois_batch_launch(ctx, oj, 1))
        sj = (SR.SboJob * 1)()
        sj[0].stats, sj[0].ref_stats, sj[0].chroma, sj[0].detect, sj[0].histogram = (put(srec[k]) for k in side)
        for k, z in enumerate(srec["zz"]):
            sj[0].zz[k] = put(z)
        sj[0].me, sj[0].ois, sj[0].cur_slot = None, None, 1
        sj[0].zz_count, sj[0].slice_type, sj[0].temporal_layer_index, sj[0].is_used_as_reference, sj[0].want_qpm = len(srec["zz"]), 2, 0, 1, 1
        st = SR.SboArrays(sbo_lcu.ptr.value, sbo_pic.ptr.value)
        before = markers(lib, ctx)
        ok(lib, lib.svt_amd_source_ops_batch_launch(ctx, sj, 1, w, h, 4, 4, C.byref(st)))
        sbo_waits = markers(lib, ctx)[1] - before[1]
        j = (M.MdcJob * 1)()
        M.fill_scalars(j[0], jb, LAMBDA, SPLIT_BITS)
        j[0].me, j[0].cur_slot = None, 1
        j[0].stats, j[0].detect, j[0].sbo_lcu, j[0].sbo_pic = sj[0].stats, sj[0].detect, sbo_lcu.ptr.value, sbo_pic.ptr.value
        j[0].pic_detect, j[0].noise_pic, j[0].stationary_edge = put(rec["pic_detect"]), put(rec["noise_pic"]), put(rec["stationary_edge"])
        t = outs[0].table()
        before = markers(lib, ctx)
        ok(lib, launch(lib, ctx, j, 1, w, h, t))
        after = markers(lib, ctx)
        assert after[1] - before[1] == sbo_waits and after[0] == before[0], (before, after, sbo_waits)
        lcu, pic = outs[0].download()                               # the first wait of the chain
        me = np.zeros(nl, S.ME_LCU_DTYPE)
        ok(lib, lib.svt_amd_me_picture_fetch(ctx, 1, me.ctypes.data))
        assert me["pu"]["distortion"][:, 0, 0].any()
        me_dev.put(me)
        j[0].me, j[0].cur_slot = me_dev.ptr.value, -1
        t = outs[1].table()
        ok(lib, launch(lib, ctx, j, 1, w, h, t))
        lcu_p, pic_p = outs[1].download()
        assert lcu.tobytes() == lcu_p.tobytes() and pic.tobytes() == pic_p.tobytes()
        chain = dict(rec, me=me, stats=srec["stats"], detect=srec["detect"], sbo_lcu=sbo_lcu.get().view(SR.SBO_LCU_DTYPE), sbo_pic=sbo_pic.get().view(SR.SBO_PIC_DTYPE))
        want_lcu, want_pic, _ = N.md_config(w, h, chain, jb, LAMBDA, SPLIT_BITS)
        same(lcu[0], pic[0], want_lcu, want_pic, "chain")
    finally:
        for b in outs + [dev, sbo_lcu, sbo_pic, me_dev]:
            b.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_entry_and_queue_nothing(lib):
    name = "whole_256x128"
    w, h, seed, jobs = R.CASES[name]
    ctx = make_context(lib, w, h, 3)
    g, pics = fixture_pictures(lib, ctx, name)
    out = Results(lib, ctx, 2, w, h)
    t = out.table()
    upload(lib, ctx, 0, S.gen_luma("motion", w, h, 0, 5))          # slot 0: a picture of the batch's size, but no ME records
    upload(lib, ctx, 1, S.gen_luma("motion", 192, 128, 0, 5))      # slot 1: a picture of another size; slot 2: no picture
    ok(lib, lib.svt_amd_synchronize(ctx))
    before = markers(lib, ctx)

    def bad(change, what, **launch_args):
        pair = (M.MdcJob * 2)()
        pair[0], pair[1] = pics.job(0), pics.job(1)
        change(pair[1])
        args = dict(n=2, w=w, h=h, table=t)
        args.update(launch_args)
        refused(lib, launch(lib, ctx, pair, args["n"], args["w"], args["h"], args["table"]), M.ENTRY, what)
        assert b"job 1" in lib.svt_amd_last_error() or launch_args, lib.svt_amd_last_error()

    def from_slot(slot):
        def change(j):
            j.me, j.cur_slot = None, slot
        return change

    try:
        for field in ("stats", "detect", "sbo_lcu", "sbo_pic", "pic_detect", "noise_pic"):
            bad(lambda j: setattr(j, field, None), field)
        bad(lambda j: setattr(j, "slice_type", 0), "an I picture")
        bad(lambda j: setattr(j, "slice_type", 3), "slice type")
        bad(lambda j: setattr(j, "temporal_layer_index", 6), "layer")
        bad(lambda j: setattr(j, "hierarchical_levels", 6), "hierarchical levels")
        bad(lambda j: setattr(j, "resolution_class", 4), "class")
        bad(lambda j: setattr(j, "depth_mode", 6), "depth mode")
        bad(lambda j: setattr(j, "qp", 52), "QP")
        bad(from_slot(-1), "no such slot")
        bad(from_slot(3), "no such slot")
        bad(from_slot(2), "a slot without a picture")
        bad(from_slot(1), "a slot of another size")
        bad(from_slot(0), "incomplete ME records")
        bad(lambda j: None, "more than 13,854 LCUs", w=7552, h=7552)   # 118 x 118 = 13,924
        bad(lambda j: None, "larger than the context", w=w + 64)
        bad(lambda j: None, "no lcu array", table=M.MdcArrays(None, out.pic.ptr.value))
        bad(lambda j: None, "no picture array", table=M.MdcArrays(out.lcu.ptr.value, None))
        for n in (0, -1, M.MAX_BATCH + 1):
            bad(lambda j: None, "job count", n=n)
        assert markers(lib, ctx) == before                          # no completion record, no wait
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert out.untouched()
        # the stationary-edge pointer alone may be NULL
        pair = pics.job_array([0, 1])
        pair[1].stationary_edge = None
        ok(lib, launch(lib, ctx, pair, 2, w, h, t))
        lcu, pic = out.download()
        want_lcu, want_pic, _ = N.md_config(w, h, dict(pics.recs[1], stationary_edge=None), jobs[1], *pics.tabs[1])
        same(lcu[1], pic[1], want_lcu, want_pic, "stationary_edge NULL")
        same(lcu[0], pic[0], g["lcu"][0], g["picture"][0], "beside it")
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 7. a batch of one and the largest batch -----------------------------------------------------------------------------------------------------------

def test_a_batch_of_one_and_the_largest_batch(lib):
    name = "aura_192x192"
    w, h, seed, jobs = R.CASES[name]
    ctx = make_context(lib, w, h, 1)
    g, pics = fixture_pictures(lib, ctx, name)
    out = Results(lib, ctx, M.MAX_BATCH, w, h)
    t = out.table()
    try:
        lcu, pic = run(lib, ctx, pics, [4])
        same(lcu[0], pic[0], g["lcu"][4], g["picture"][4], "a batch of one")
        order = [i % len(jobs) for i in range(M.MAX_BATCH)]
        ok(lib, launch(lib, ctx, pics.job_array(order), M.MAX_BATCH, w, h, t))
        lcu, pic = out.download()
        for k in (0, 1, 127, 254, 255):
            same(lcu[k], pic[k], g["lcu"][order[k]], g["picture"][order[k]], ("256", k))
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)
