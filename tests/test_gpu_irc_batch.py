"""The batched initial rate control on the device (include/svt_hevc_amd.h "Batched initial rate control"; svt-hevc_amd/csrc/irc_kernels.hip) through the C-ABI:
svt_amd_initial_rc_batch_launch against the records the REFERENCE's own functions left for the seeded sequences (tests/golden/irc_*.npz), against the
restatement (tests/irc_numpy.py, pinned on the same files by tests/test_irc_cpu.py) on a further seeded sequence at the shapes where the kernels take another
path, and chained on one lane behind ME, OIS, the side statistics and the detectors with the ME records read where they lie and the mode-decision
configuration reading the stationary-edge bytes where this entry left them.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import irc_numpy as N
import irc_records as R
import irclib as M
import mdc_numpy as MN
import mdc_records as MR
import mdclib as MM
import pa_detect_numpy as PN
import pa_detect_pictures as P
import sbo_records as SR
import sidelib as L
import svtlib as S
from gpu_util import default_params, upload
from pa_batch_util import DeviceBuffer, is_sentinel, make_context, markers, ok, refused, round_up as _up
from test_irc_cpu import CASES, load_case, same

pytestmark = pytest.mark.gpu
KINDS = ("checks", "motion", "lcu", "stationary_edge", "pm_stationary_edge", "picture")


@pytest.fixture(scope="module")
def lib(product):
    return M.declare(product)


def edge_bytes(nl):
    return (nl + 63) // 64 * 64


class Results:
    """the six output arrays of an n-picture batch, filled with SENTINEL"""

    def __init__(self, lib, ctx, n, w, h):
        self.lib, self.n, self.nl = lib, n, S.lcu_count(w, h)
        self.sizes = dict(checks=self.nl * R.CHECKS_DTYPE.itemsize, motion=R.MOTION_DTYPE.itemsize, lcu=self.nl * R.IRC_LCU_DTYPE.itemsize,
                          stationary_edge=edge_bytes(self.nl), pm_stationary_edge=edge_bytes(self.nl), picture=R.IRC_PIC_DTYPE.itemsize)
        assert [self.sizes[k] for k in KINDS] == [lib.svt_amd_initial_rc_bytes(w, h, which) for which in range(6)]
        self.buf = {k: DeviceBuffer(lib, ctx, n * self.sizes[k]) for k in KINDS}

    def table(self, first=0):
        """the table of a batch whose picture 0 lands at place `first` of the arrays"""
        return M.IrcArrays(*[self.buf[k].at(first * self.sizes[k]) for k in KINDS])

    def at(self, kind, place):
        return self.buf[kind].at(place * self.sizes[kind])

    def raw(self):
        return {k: self.buf[k].get().reshape(self.n, -1) for k in KINDS}

    def download(self):
        """-> the arrays as irc_numpy.initial_rc has them; the tail of the stationary-edge bytes is checked and cut"""
        raw = self.raw()
        out = dict(checks=raw["checks"].view(R.CHECKS_DTYPE), motion=raw["motion"].view(R.MOTION_DTYPE)[:, 0], lcu=raw["lcu"].view(R.IRC_LCU_DTYPE),
                   picture=raw["picture"].view(R.IRC_PIC_DTYPE)[:, 0])
        for k in ("stationary_edge", "pm_stationary_edge"):
            assert not raw[k][:, self.nl:].any(), (k, "tail")
            out[k] = raw[k][:, :self.nl]
        for k in ("motion", "lcu", "picture"):
            assert not out[k]["pad"].any(), (k, "pad bytes")
        assert not out["picture"]["pad0"].any()
        return out

    def untouched(self):
        return all(is_sentinel(b.get()) for b in self.buf.values())

    def free(self):
        for b in self.buf.values():
            b.free()


class Sequence:
    """the records of the pictures of a sequence in device memory, and the jobs that point at them"""

    def __init__(self, lib, ctx, w, h, cls, seq, recs):
        self.lib, self.ctx, self.w, self.h, self.cls, self.seq, self.recs = lib, ctx, w, h, cls, seq, recs
        self.lists = N.sequence_lists(seq)
        self.keep, self.where = [], []
        self.dev = DeviceBuffer(lib, ctx, sum(_up(r[k].nbytes) for r in recs for k in ("me", "stats", "detect")))
        off = 0
        for r in recs:
            at = {}
            for k in ("me", "stats", "detect"):
                a = np.ascontiguousarray(r[k])
                self.keep.append(a)
                self.dev.put(a, off)
                at[k], off = self.dev.at(off), off + _up(a.nbytes)
            self.where.append(at)

    def job(self, i, place_of):
        """the job of picture i; place_of(k) -> (Results, place) that hold - or will hold - the checks and the motion record of picture k"""
        def at(kind, k):
            if kind in ("stats", "detect"):
                return self.where[k][kind]
            res, place = place_of(k)
            return res.at(kind, place)
        j = M.IrcJob()
        j.me, j.stats, j.cur_slot = self.where[i]["me"], self.where[i]["stats"], -1
        return M.fill_job(j, self.seq["pics"][i], self.cls, self.lists[i], at)

    def job_array(self, order, place_of):
        jobs = (M.IrcJob * len(order))()
        for k, i in enumerate(order):
            jobs[k] = self.job(i, place_of)
        return jobs

    def free(self):
        self.dev.free()


def launch(lib, ctx, jobs, n, w, h, table):
    return lib.svt_amd_initial_rc_batch_launch(ctx, jobs, n, w, h, C.byref(table))


def run_whole(lib, ctx, sq, order=None):
    """one batch of every picture of the sequence in the order given: the windows point into the batch's own arrays -> the arrays, picture order[k] at place k"""
    order = list(range(len(sq.recs))) if order is None else order
    out = Results(lib, ctx, len(order), sq.w, sq.h)
    t = out.table()
    ok(lib, launch(lib, ctx, sq.job_array(order, lambda k: (out, order.index(k))), len(order), sq.w, sq.h, t))
    return out


def pick(arrays, places):
    return {k: arrays[k][places] for k in KINDS}


def case_sequence(lib, ctx, name):
    w, h, cls, seed, seq = R.CASES[name]
    return Sequence(lib, ctx, w, h, cls, seq, R.case_inputs(name))


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_fixture_gives_what_the_reference_computed(lib, name):
    w, h, cls, seed, seq = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    sq = case_sequence(lib, ctx, name)
    out = run_whole(lib, ctx, sq)                                 # one batch of all the case's pictures
    try:
        same(out.download(), g, name)
    finally:
        out.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)


def test_an_i_picture_without_a_look_ahead_reads_no_me_records(lib):
    """the last picture of a sequence that ends in an I picture: the raw flags of an all-zero motion record, the reset homogeneity records, no window - and
    neither `me` nor `cur_slot` is looked at: a batch of that picture alone, with no ME pointer and a slot the context does not have"""
    name = "ends_intra_128x64"
    w, h, cls, seed, seq = R.CASES[name]
    g = load_case(name)
    last = len(seq["pics"]) - 1
    ctx = make_context(lib, w, h, 1)
    sq = case_sequence(lib, ctx, name)
    out = Results(lib, ctx, 1, w, h)
    try:
        assert seq["pics"][last]["slice_type"] == R.I and not sq.lists[last]["look_ahead"]
        before = markers(lib, ctx)
        jobs = sq.job_array([last], lambda k: (out, 0))
        jobs[0].me, jobs[0].cur_slot = None, 7
        t = out.table()
        ok(lib, launch(lib, ctx, jobs, 1, w, h, t))
        assert markers(lib, ctx)[1] == before[1]                   # no wait on a slot
        got = out.download()
        same(got, pick(g, [last]), name)
        assert not any(got["motion"].tobytes()) and not got["lcu"]["motion_votes"].any()
        assert (got["lcu"]["var_of_var_over_time"] == 0xFFFFFFFFFFFFFFFF).all() and not got["lcu"]["homogeneous_over_time"].any()
        assert got["picture"]["is_pan"][0] == 0 and got["picture"]["is_tilt"][0] == 0 and got["picture"]["homogeneity_percentage"][0] == 0
    finally:
        out.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 2. a further seeded sequence against the restatement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,seed", [(64, 64, 43), (128, 64, 47), (192, 128, 53), (960, 136, 59), (2112, 1152, 61)])
def test_seeded_variants_match_the_restatement(lib, w, h, seed):
    """one LCU; two LCUs - every neighbour test meets a picture edge; a 3 x 2 grid; a partial bottom row under two complete ones; 594 LCUs - 149 workgroups of
    vote totals, ten waves of the finish kernel at work"""
    cls = 3 if w == 2112 else 2 if w == 960 else 0
    seq = R._usual_jobs()
    recs = R.make_inputs(w, h, cls, seed, seq)
    ctx = make_context(lib, w, h, 1)
    sq = Sequence(lib, ctx, w, h, cls, seq, recs)
    out = run_whole(lib, ctx, sq)
    try:
        same(out.download(), N.initial_rc(w, h, cls, seq, recs, sq.lists), (w, h))
    finally:
        out.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 3. a mixed batch in both orders ---------------------------------------------------------------------------------------------------------------

def test_a_mixed_batch_in_both_orders_equals_the_single_launches(lib):
    """I, P and B pictures, with and without a look-ahead, a scene change inside the windows: one batch forwards, one backwards, and one batch per picture -
    the last picture first, so that every window entry is written when its reader is queued - byte for byte"""
    name = "scene_256x192"
    w, h, cls, seed, seq = R.CASES[name]
    g = load_case(name)
    count = len(seq["pics"])
    ctx = make_context(lib, w, h, 1)
    sq = case_sequence(lib, ctx, name)
    single = Results(lib, ctx, count, w, h)
    outs = [single]
    try:
        for i in reversed(range(count)):
            t = single.table(i)
            ok(lib, launch(lib, ctx, sq.job_array([i], lambda k: (single, k)), 1, w, h, t))
        want = single.raw()
        same(single.download(), g, "single launches")
        for order in (list(range(count)), list(reversed(range(count)))):
            outs.append(run_whole(lib, ctx, sq, order))
            got = outs[-1].raw()
            for k, i in enumerate(order):
                for kind in KINDS:
                    assert got[kind][k].tobytes() == want[kind][i].tobytes(), (order[0], i, kind)
    finally:
        for o in outs:
            o.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 4. two batches back to back --------------------------------------------------------------------------------------------------------------------

def test_two_batches_back_to_back_on_one_lane(lib):
    """the second batch is queued while the first may still run: it reuses the descriptor table and the scratch (vote totals, vote and flag bytes) of the first -
    stored into, never accumulated - and its windows point into the arrays the first batch writes"""
    name = "corners_704x640"
    w, h, cls, seed, seq = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    sq = case_sequence(lib, ctx, name)
    later, earlier = list(range(9, 20)), list(range(9))
    outs = [Results(lib, ctx, len(later), w, h), Results(lib, ctx, len(earlier), w, h)]
    place_of = lambda k: (outs[0], k - 9) if k >= 9 else (outs[1], k)  # noqa: E731
    try:
        for order, out in zip((later, earlier), outs):
            t = out.table()
            ok(lib, launch(lib, ctx, sq.job_array(order, place_of), len(order), w, h, t))
        for order, out in zip((later, earlier), outs):
            same(out.download(), pick(g, order), order[0])
    finally:
        for out in outs:
            out.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 5. the chain on one lane -------------------------------------------------------------------------------------------------------------------------

def test_chain_on_one_lane_reads_the_records_where_they_lie(lib):
    """upload, ME, OIS, side statistics, chroma means, detectors, the source-based operations, this entry with me = NULL and the mode-decision configuration
    reading this entry's stationary_edge bytes in place, queued on one lane with nothing downloaded in between.  This entry's bytes equal the run with the ME
    records given by pointer and the restatement on the downloaded records; it waits as often as the source-ops consumer in front of it did - not at all;
    the mode-decision configuration's records equal its restatement on the downloaded inputs"""
    w, h, rw, rh, seed = 320, 256, 4, 4, 71
    nl, plane = S.lcu_count(w, h), (w // 2) * (h // 2)
    MM.declare(SR.declare(PN.declare(L.declare(lib))))
    ctx = make_context(lib, w, h, 4)
    frames = [P.gen_luma("motion", w, h, t, seed) for t in range(4)]
    cb, cr = (np.ascontiguousarray(a) for a in P.gen_chroma("motion", w, h, 1, seed))
    sizes = L.numpy_sizes(w, h, rw, rh)
    mjb = MR.job(MR.B, 0, 1, 8, 2, qp=30, noise=3, stationary="some")
    mrec = MR.make_inputs(w, h, seed, 0, mjb)
    buf = dict(stats=DeviceBuffer(lib, ctx, 3 * sizes[L.BLOCK_STATS]), zz=DeviceBuffer(lib, ctx, 3 * sizes[L.ZZ_SAD]), hist=DeviceBuffer(lib, ctx, 3 * sizes[L.HISTOGRAM]),
               planes=DeviceBuffer(lib, ctx, 2 * plane), means=DeviceBuffer(lib, ctx, nl * 48), dlcu=DeviceBuffer(lib, ctx, nl * 48), dpic=DeviceBuffer(lib, ctx, 8),
               sbo_lcu=DeviceBuffer(lib, ctx, nl * SR.SBO_LCU_DTYPE.itemsize), sbo_pic=DeviceBuffer(lib, ctx, SR.SBO_PIC_DTYPE.itemsize),
               noise=DeviceBuffer(lib, ctx, 256), me=DeviceBuffer(lib, ctx, nl * S.ME_LCU_DTYPE.itemsize),
               mdc_lcu=DeviceBuffer(lib, ctx, nl * MR.MDC_LCU_DTYPE.itemsize), mdc_pic=DeviceBuffer(lib, ctx, MR.MDC_PIC_DTYPE.itemsize))
    outs = [Results(lib, ctx, 1, w, h) for _ in range(2)]
    noise_pic = np.ascontiguousarray(mrec["noise_pic"])
    # the picture's window: itself three times over (the entry takes any list), four frames to check - the threshold is 0
    lists = dict(look_ahead=1, frames_to_check=4, edge=[0], hom=[0, 0, 0], pan=[0])
    p = dict(R.pic(R.B, 0), poc=0, eos=0)
    try:
        for s, f in enumerate(frames):
            upload(lib, ctx, s, f)
        buf["planes"].put(cb, 0), buf["planes"].put(cr, plane), buf["noise"].put(noise_pic)
        mj, oj = (S.MeJob * 1)(), (S.OisJob * 1)()
        mj[0].params, mj[0].cur_slot = default_params(w, h, num_lists=2, temporal_layer_index=0, cu8x8_mode=0), 1
        mj[0].ref_slot[0], mj[0].ref_slot[1] = 0, 2
        op = S.OisParams()
        op.luma_width, op.luma_height, op.ois_th_set, op.temporal_layer_index = w, h, 1, 0
        oj[0].params, oj[0].cur_slot = op, 1
        ok(lib, lib.svt_amd_me_batch_launch(ctx, mj, 1))
        ok(lib, lib.svt_amd_ois_batch_launch(ctx, oj, 1))
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
        sj = (SR.SboJob * 1)()
        sj[0].stats, sj[0].ref_stats, sj[0].chroma, sj[0].detect, sj[0].histogram = buf["stats"].at(0), buf["stats"].at(sizes[L.BLOCK_STATS]), buf["means"].at(0), buf["dlcu"].at(0), buf["hist"].at(0)
        for k in range(3):
            sj[0].zz[k] = buf["zz"].at(k * sizes[L.ZZ_SAD])
        sj[0].me, sj[0].ois, sj[0].cur_slot = None, None, 1
        sj[0].zz_count, sj[0].slice_type, sj[0].temporal_layer_index, sj[0].is_used_as_reference, sj[0].want_qpm = 3, 2, 0, 1, 1
        sbt = SR.SboArrays(buf["sbo_lcu"].ptr.value, buf["sbo_pic"].ptr.value)
        before = markers(lib, ctx)
        ok(lib, lib.svt_amd_source_ops_batch_launch(ctx, sj, 1, w, h, rw, rh, C.byref(sbt)))
        sbo_waits = markers(lib, ctx)[1] - before[1]
        assert sbo_waits == 0                                        # the producers ran on this very lane

        def irc_job(out):
            def at(kind, k):
                return {"stats": buf["stats"].at(0), "detect": buf["dlcu"].at(0)}[kind] if kind in ("stats", "detect") else out.at(kind, 0)
            j = (M.IrcJob * 1)()
            j[0].stats = buf["stats"].at(0)
            M.fill_job(j[0], p, 0, lists, at)
            return j
        j = irc_job(outs[0])
        j[0].me, j[0].cur_slot = None, 1
        t = outs[0].table()
        before = markers(lib, ctx)
        ok(lib, launch(lib, ctx, j, 1, w, h, t))
        after = markers(lib, ctx)
        assert after[1] - before[1] == sbo_waits and after[0] == before[0], (before, after, sbo_waits)
        dj2 = (MM.MdcJob * 1)()
        MM.fill_scalars(dj2[0], mjb, 261, [12171, 78934])
        dj2[0].me, dj2[0].cur_slot = None, 1
        dj2[0].stats, dj2[0].detect, dj2[0].sbo_lcu, dj2[0].sbo_pic = buf["stats"].at(0), buf["dlcu"].at(0), buf["sbo_lcu"].ptr.value, buf["sbo_pic"].ptr.value
        dj2[0].pic_detect, dj2[0].noise_pic, dj2[0].stationary_edge = buf["dpic"].ptr.value, buf["noise"].ptr.value, outs[0].at("stationary_edge", 0)
        mt = MM.MdcArrays(buf["mdc_lcu"].ptr.value, buf["mdc_pic"].ptr.value)
        ok(lib, lib.svt_amd_md_config_batch_launch(ctx, dj2, 1, w, h, C.byref(mt)))
        got = outs[0].download()                                    # the first wait of the chain
        raw = outs[0].raw()
        me = np.zeros(nl, S.ME_LCU_DTYPE)
        ok(lib, lib.svt_amd_me_picture_fetch(ctx, 1, me.ctypes.data))
        assert me["pu"]["distortion"][:, 0, 0].any()
        buf["me"].put(me)
        j = irc_job(outs[1])
        j[0].me, j[0].cur_slot = buf["me"].ptr.value, -1
        t = outs[1].table()
        ok(lib, launch(lib, ctx, j, 1, w, h, t))
        raw_p = outs[1].raw()
        for kind in KINDS:
            assert raw[kind].tobytes() == raw_p[kind].tobytes(), kind
        stats = buf["stats"].get().view(S.PA_LCU_STATS_DTYPE).reshape(3, nl)[0]
        detect = buf["dlcu"].get().view(PN.LCU_DETECT_DTYPE)
        seq = dict(pics=[dict(p, eos=0)])
        same(got, N.initial_rc(w, h, 0, seq, [dict(me=me, stats=stats, detect=detect)], [lists]), "chain")
        assert got["checks"]["check2"].all() and got["lcu"]["var_of_var_over_time"].max() == 0   # three times the same variance: no spread over time
        chain = dict(mrec, me=me, stats=stats, detect=detect, sbo_lcu=buf["sbo_lcu"].get().view(SR.SBO_LCU_DTYPE), sbo_pic=buf["sbo_pic"].get().view(SR.SBO_PIC_DTYPE),
                     pic_detect=buf["dpic"].get().view(MR.PIC_DETECT_DTYPE), stationary_edge=got["stationary_edge"][0])
        want_lcu, want_pic, _ = MN.md_config(w, h, chain, mjb, 261, [12171, 78934])
        mdc_lcu, mdc_pic = buf["mdc_lcu"].get().view(MR.MDC_LCU_DTYPE), buf["mdc_pic"].get().view(MR.MDC_PIC_DTYPE)
        for f in MR.LCU_FIELDS:
            assert np.array_equal(mdc_lcu[f], want_lcu[f]), ("mode-decision configuration", f)
        for f in MR.PIC_FIELDS:
            assert np.array_equal(mdc_pic[f][0], want_pic[f]), ("mode-decision configuration", f)
    finally:
        for b in list(buf.values()) + outs:
            b.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_entry_and_queue_nothing(lib):
    name = "scene_256x192"
    w, h, cls, seed, seq = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 3)
    sq = case_sequence(lib, ctx, name)
    filled = run_whole(lib, ctx, sq)                               # the window entries of pictures 3 and 4: a batch that ran
    out = Results(lib, ctx, 2, w, h)
    t = out.table()
    upload(lib, ctx, 0, S.gen_luma("motion", w, h, 0, 5))          # slot 0: a picture of the batch's size, but no ME records
    upload(lib, ctx, 1, S.gen_luma("motion", 192, 128, 0, 5))      # slot 1: a picture of another size; slot 2: no picture
    ok(lib, lib.svt_amd_synchronize(ctx))
    before = markers(lib, ctx)
    place_of = lambda k: (filled, k)  # noqa: E731

    def bad(change, what, i=4, **launch_args):
        pair = (M.IrcJob * 2)()
        pair[0], pair[1] = sq.job(3, place_of), sq.job(i, place_of)
        change(pair[1])
        args = dict(n=2, w=w, h=h, table=t)
        args.update(launch_args)
        refused(lib, launch(lib, ctx, pair, args["n"], args["w"], args["h"], args["table"]), M.ENTRY, what)
        assert b"job 1" in lib.svt_amd_last_error() or launch_args, lib.svt_amd_last_error()

    def from_slot(slot):
        def change(j):
            j.me, j.cur_slot = None, slot
        return change

    def entry(field, k):
        def change(j):
            getattr(j, field)[k] = None
        return change

    def table_without(kind):
        ptrs = [out.at(k, 0) for k in KINDS]
        ptrs[KINDS.index(kind)] = None
        return M.IrcArrays(*ptrs)

    try:
        assert sq.lists[4]["edge"] and len(sq.lists[4]["hom"]) >= 1 and len(sq.lists[4]["pan"]) >= 2 and not sq.lists[13]["look_ahead"]
        bad(lambda j: setattr(j, "stats", None), "stats")
        bad(lambda j: setattr(j, "edge_count", 5), "edge_count")
        bad(lambda j: setattr(j, "hom_count", 17), "hom_count")
        bad(lambda j: setattr(j, "pan_count", 9), "pan_count")
        bad(entry("edge_checks", 0), "a NULL checks entry")
        bad(entry("edge_detect", 0), "a NULL detect entry")
        bad(entry("hom_stats", 0), "a NULL statistics entry")
        bad(entry("pan_motion", 1), "a NULL motion entry")
        for field in ("edge_count", "hom_count", "pan_count"):       # the last picture has no look-ahead: any list is one too many
            bad(lambda j: setattr(j, field, 1), field + " without a look-ahead", i=13)
        bad(lambda j: setattr(j, "frames_to_check", 2), "frames_to_check without a look-ahead", i=13)
        bad(lambda j: setattr(j, "frames_to_check", 0), "frames_to_check")
        bad(lambda j: setattr(j, "frames_to_check", 18), "frames_to_check")
        bad(lambda j: setattr(j, "slice_type", 3), "slice type")
        bad(lambda j: setattr(j, "temporal_layer_index", 4), "a layer above the levels")
        bad(lambda j: setattr(j, "hierarchical_levels", 6), "hierarchical levels")
        bad(lambda j: setattr(j, "resolution_class", 4), "class")
        bad(from_slot(-1), "no such slot")
        bad(from_slot(3), "no such slot")
        bad(from_slot(2), "a slot without a picture")
        bad(from_slot(1), "a slot of another size")
        bad(from_slot(0), "incomplete ME records")
        bad(lambda j: None, "more than 16,384 LCUs", w=8256, h=8192)   # 129 x 128 = 16,512
        bad(lambda j: None, "larger than the context", w=w + 64)
        for kind in KINDS:
            bad(lambda j: None, "no %s array" % kind, table=table_without(kind))
        for n in (0, -1, M.MAX_BATCH + 1):
            bad(lambda j: None, "job count", n=n)
        assert markers(lib, ctx) == before                          # no completion record, no wait
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert out.untouched()
        # an I picture of layer 0 reads no ME records: neither the pointer nor the slot is looked at
        assert seq["pics"][5]["slice_type"] == R.I and seq["pics"][5]["layer"] == 0
        pair = (M.IrcJob * 2)()
        pair[0], pair[1] = sq.job(3, place_of), sq.job(5, place_of)
        pair[1].me, pair[1].cur_slot = None, 7
        ok(lib, launch(lib, ctx, pair, 2, w, h, t))
        same(out.download(), pick(g, [3, 5]), "an I picture without ME records")
    finally:
        out.free()
        filled.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 7. a batch of one and the largest batch -----------------------------------------------------------------------------------------------------------

def test_a_batch_of_one_and_the_largest_batch(lib):
    name = "tail_192x128"
    w, h, cls, seed, seq = R.CASES[name]
    g = load_case(name)
    count = len(seq["pics"])
    ctx = make_context(lib, w, h, 1)
    sq = case_sequence(lib, ctx, name)
    filled = run_whole(lib, ctx, sq)
    one, big = Results(lib, ctx, 1, w, h), Results(lib, ctx, M.MAX_BATCH, w, h)
    place_of = lambda k: (filled, k)  # noqa: E731
    try:
        t = one.table()
        ok(lib, launch(lib, ctx, sq.job_array([2], place_of), 1, w, h, t))
        same(one.download(), pick(g, [2]), "a batch of one")
        order = [i % count for i in range(M.MAX_BATCH)]
        t = big.table()
        ok(lib, launch(lib, ctx, sq.job_array(order, place_of), M.MAX_BATCH, w, h, t))
        got = big.download()
        places = [0, 1, 19, 127, 254, 255]
        same(pick(got, places), pick(g, [order[k] for k in places]), "256")
    finally:
        for o in (one, big, filled):
            o.free()
        sq.free()
        lib.svt_amd_context_destroy(ctx)
