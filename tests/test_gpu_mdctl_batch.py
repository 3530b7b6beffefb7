"""The mode decision's per-LCU controls on the device (include/svt_hevc_amd.h "Batched mode-decision LCU controls"; svt-hevc_amd/csrc/mdctl_kernels.hip) through
the C-ABI.  Part A: svt_amd_md_controls_batch_launch against the records the REFERENCE left through svt_md_fill_lcu for the seeded records
(tests/golden/mdctl_*.npz), against the restatement (tests/mdctl_numpy.py, pinned on the same files by tests/test_mdctl_cpu.py) at the shapes where the kernel
takes another path, and chained on one lane behind every batch in front of it.  Part B: svt_amd_md_picture_set_controls - the mode-decision call reads a bound
device array in place and decides, byte for byte, what it decides from the same records passed as host memory.  Every comparison is bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import irc_records as IR
import irclib as IM
import mdc_records as MR
import mdclib as MM
import mdctl_numpy as N
import mdctl_records as R
import mdctllib as M
import pa_detect_numpy as PN
import pa_detect_pictures as P
import pa_noise_numpy as NZ
import sbo_records as SR
import sidelib as L
import svtlib as S
from gpu_util import default_params, upload
from pa_batch_util import BAD_PARAM, SENTINEL, DeviceBuffer, is_sentinel, make_context, markers, ok, refused, round_up as _up
from test_mdctl_cpu import CASES, load_case, same
from test_oracle_md_golden import inter_inputs

pytestmark = pytest.mark.gpu
REC = R.MD_LCU_DTYPE.itemsize          # 191
GUARD = 256                            # sentinel bytes kept behind the last record of an output array
KINDS = M.POINTER_FIELDS


@pytest.fixture(scope="module")
def lib(product):
    return M.declare(product)


class Pictures:
    """the records of the pictures of a case in device memory, and the jobs that point at them"""

    def __init__(self, lib, ctx, w, h, jobs, recs):
        self.lib, self.ctx, self.w, self.h, self.jobs, self.recs = lib, ctx, w, h, jobs, recs
        self.keep, self.where = [], []
        self.dev = DeviceBuffer(lib, ctx, sum(_up(r[k].nbytes) for r in recs for k in KINDS if r[k] is not None) + 256)
        off = 0
        for r in recs:
            at = {}
            for k in KINDS:
                if r[k] is None:
                    at[k] = None
                    continue
                a = np.ascontiguousarray(r[k])
                self.keep.append(a)
                self.dev.put(a, off)
                at[k], off = self.dev.at(off), off + _up(a.nbytes)
            self.where.append(at)

    def job(self, i):
        return M.fill_job(M.MdCtlJob(), self.jobs[i], lambda kind: self.where[i][kind])

    def job_array(self, order):
        jobs = (M.MdCtlJob * len(order))()
        for k, i in enumerate(order):
            jobs[k] = self.job(i)
        return jobs

    def free(self):
        self.dev.free()


class Out:
    """the output array of an n-picture batch and GUARD bytes behind it, filled with SENTINEL"""

    def __init__(self, lib, ctx, n, w, h):
        self.lib, self.n, self.nl = lib, n, S.lcu_count(w, h)
        assert lib.svt_amd_md_controls_bytes(w, h, M.MDCTL_LCU) == self.nl * REC
        self.buf = DeviceBuffer(lib, ctx, n * self.nl * REC + GUARD)

    def at(self, place=0):
        return self.buf.at(place * self.nl * REC)

    def raw(self):
        return self.buf.get()

    def download(self):
        """-> MD_LCU_DTYPE[n][lcus]; the bytes behind the last record must be untouched"""
        raw = self.raw()
        assert is_sentinel(raw[self.n * self.nl * REC:]), "bytes behind the last record"
        return raw[:self.n * self.nl * REC].view(R.MD_LCU_DTYPE).reshape(self.n, self.nl)

    def untouched(self):
        return is_sentinel(self.raw())

    def free(self):
        self.buf.free()


def launch(lib, ctx, jobs, n, w, h, out_ptr):
    return lib.svt_amd_md_controls_batch_launch(ctx, jobs, n, w, h, C.c_void_p(out_ptr))


def run_whole(lib, ctx, pics, order=None):
    order = list(range(len(pics.recs))) if order is None else order
    out = Out(lib, ctx, len(order), pics.w, pics.h)
    ok(lib, launch(lib, ctx, pics.job_array(order), len(order), pics.w, pics.h, out.at()))
    return out


def case_pictures(lib, ctx, name):
    w, h, seed, jobs = R.CASES[name]
    return Pictures(lib, ctx, w, h, jobs, R.case_inputs(name))


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_fixture_gives_what_the_reference_computed(lib, name):
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = case_pictures(lib, ctx, name)
    out = run_whole(lib, ctx, pics)                               # one batch of all the case's pictures
    try:
        same(out.download(), g["lcu"], name)
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 2. further seeded pictures against the restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,seed,tiles", [(64, 64, 43, (1, 1)), (128, 64, 47, (2, 1)), (192, 128, 53, (3, 2)), (960, 136, 59, (4, 3)), (2112, 1152, 61, (5, 7))])
def test_seeded_variants_match_the_restatement(lib, w, h, seed, tiles):
    """one LCU; two LCUs, a tile each; a 3 x 2 grid of one-LCU tiles; a partial bottom row; 33 x 18 LCUs - the last workgroup holds two LCUs"""
    cls = 3 if w == 2112 else 2 if w == 960 else 0
    jobs = R._usual_jobs(cls, tiles)
    recs = [R.make_inputs(w, h, seed, i, jb) for i, jb in enumerate(jobs)]
    ctx = make_context(lib, w, h, 1)
    pics = Pictures(lib, ctx, w, h, jobs, recs)
    out = run_whole(lib, ctx, pics)
    try:
        same(out.download(), np.stack([N.md_controls(w, h, rec, jb) for jb, rec in zip(jobs, recs)]), (w, h))
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 3. a mixed batch in both orders ---------------------------------------------------------------------------------------------------------------

def test_a_mixed_batch_in_both_orders_equals_the_single_launches(lib):
    """I, P and B jobs, with and without configuration records: one batch forwards, one backwards, and one launch a picture, byte for byte.  The records of a
    picture lie at every alignment (191 n modulo 4)"""
    name = "partial_416x240"
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    count = len(jobs)
    assert {jb["slice_type"] for jb in jobs} == {R.I, R.P, R.B} and {jb["mdc"] for jb in jobs} == {True, False}
    ctx = make_context(lib, w, h, 1)
    pics = case_pictures(lib, ctx, name)
    single = Out(lib, ctx, count, w, h)
    outs = [single]
    try:
        for i in reversed(range(count)):
            ok(lib, launch(lib, ctx, pics.job_array([i]), 1, w, h, single.at(i)))
        want = single.download()
        same(want, g["lcu"], "single launches")
        for order in (list(range(count)), list(reversed(range(count)))):
            outs.append(run_whole(lib, ctx, pics, order))
            got = outs[-1].download()
            for k, i in enumerate(order):
                assert got[k].tobytes() == want[i].tobytes(), (order[0], i)
    finally:
        for o in outs:
            o.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 4. two batches back to back --------------------------------------------------------------------------------------------------------------------

def test_two_batches_back_to_back_into_adjacent_arrays(lib):
    """the second batch is queued while the first may still run: it reuses the descriptor table through the upload ring, and its first record shares a word with
    the last record of the first batch (3 x 110 x 191 bytes is no multiple of 4: the shared word is written as bytes by both)"""
    name = "uneven_704x640"
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = case_pictures(lib, ctx, name)
    first, second = [0, 1, 2], list(range(3, len(jobs)))
    out = Out(lib, ctx, len(jobs), w, h)
    try:
        assert (len(first) * out.nl * REC) % 4 != 0
        ok(lib, launch(lib, ctx, pics.job_array(first), len(first), w, h, out.at(0)))
        ok(lib, launch(lib, ctx, pics.job_array(second), len(second), w, h, out.at(len(first))))
        same(out.download(), g["lcu"], name)
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 5. the chain on one lane -------------------------------------------------------------------------------------------------------------------------

class Chain:
    """upload, ME, OIS, side statistics, chroma means, detectors, noise, source ops, initial rate control, mode-decision configuration and the controls of one
    192 x 128 B picture queued on ONE lane, with no synchronisation and no host copy between the launches.  The controls stay in self.controls (device)."""
    W, H, RW, RH = 192, 128, 4, 4

    def __init__(self, lib, seed, chroma_level=4, depth_mode=MR.PICT_LCU_SWITCH):
        w, h, rw, rh = self.W, self.H, self.RW, self.RH
        self.lib = lib
        MM.declare(SR.declare(PN.declare(L.declare(IM.declare(lib)))))
        NZ.declare(lib)
        self.nl = nl = S.lcu_count(w, h)
        plane = (w // 2) * (h // 2)
        self.ctx = ctx = make_context(lib, w, h, 4)
        frames = [P.gen_luma("motion", w, h, t, seed) for t in range(4)]
        self.keep = [np.ascontiguousarray(a) for a in P.gen_chroma("motion", w, h, 1, seed)]
        self.sizes = sizes = L.numpy_sizes(w, h, rw, rh)
        self.mjb = MR.job(MR.B, 3, 0, 8, 0, qp=30, noise=1, stationary="some", depth_mode=depth_mode)
        self.jb = R.job(R.B, depth_mode, chroma_level, 0, tiles=(1, 1))
        self.buf = buf = dict(stats=DeviceBuffer(lib, ctx, 3 * sizes[L.BLOCK_STATS]), energy=DeviceBuffer(lib, ctx, 3 * sizes[L.AC_ENERGY]),
                              zz=DeviceBuffer(lib, ctx, 3 * sizes[L.ZZ_SAD]), hist=DeviceBuffer(lib, ctx, 3 * sizes[L.HISTOGRAM]),
                              planes=DeviceBuffer(lib, ctx, 2 * plane), means=DeviceBuffer(lib, ctx, nl * 48), dlcu=DeviceBuffer(lib, ctx, nl * 48),
                              dpic=DeviceBuffer(lib, ctx, 8), sbo_lcu=DeviceBuffer(lib, ctx, nl * SR.SBO_LCU_DTYPE.itemsize),
                              sbo_pic=DeviceBuffer(lib, ctx, SR.SBO_PIC_DTYPE.itemsize), flat=DeviceBuffer(lib, ctx, 64 * ((nl + 63) // 64)),
                              noise=DeviceBuffer(lib, ctx, 256), mdc_lcu=DeviceBuffer(lib, ctx, nl * MR.MDC_LCU_DTYPE.itemsize),
                              mdc_pic=DeviceBuffer(lib, ctx, MR.MDC_PIC_DTYPE.itemsize),
                              irc=DeviceBuffer(lib, ctx, _up(nl * 4) + 256 + _up(nl * 48) + 2 * _up(64 * ((nl + 63) // 64)) + 256))
        self.controls = Out(lib, ctx, 1, w, h)
        for s, f in enumerate(frames):
            upload(lib, ctx, s, f)
        buf["planes"].put(self.keep[0], 0), buf["planes"].put(self.keep[1], plane)
        mj, oj = (S.MeJob * 1)(), (S.OisJob * 1)()
        mj[0].params, mj[0].cur_slot = default_params(w, h, num_lists=2, temporal_layer_index=3, cu8x8_mode=0), 1
        mj[0].ref_slot[0], mj[0].ref_slot[1] = 0, 2
        op = S.OisParams()
        op.luma_width, op.luma_height, op.ois_th_set, op.temporal_layer_index = w, h, 1, 3
        oj[0].params, oj[0].cur_slot = op, 1
        ok(lib, lib.svt_amd_me_batch_launch(ctx, mj, 1))
        ok(lib, lib.svt_amd_ois_batch_launch(ctx, oj, 1))
        side = L.make_jobs([(1, 0, 1, 1, 1), (2, 1, 1, 1, 1), (3, 2, 1, 1, 1)])
        st = L.SideArrays(block_stats=buf["stats"].ptr.value, ac_energy=buf["energy"].ptr.value, zz=buf["zz"].ptr.value, histogram=buf["hist"].ptr.value)
        ok(lib, lib.svt_amd_side_stats_batch_launch(ctx, side, 3, rw, rh, C.byref(st)))
        cj = (PN.ChromaJob * 1)()
        cj[0].cb, cj[0].cr, cj[0].pitch, cj[0].want_means, cj[0].want_histogram = buf["planes"].at(0), buf["planes"].at(plane), w // 2, 1, 0
        ct = PN.ChromaArrays(buf["means"].ptr.value, None, None, None)
        ok(lib, lib.svt_amd_chroma_stats_batch_launch(ctx, cj, 1, w, h, rw, rh, C.byref(ct)))
        dj = (PN.DetectJob * 1)()
        dj[0].stats, dj[0].chroma, dj[0].want_edge16, dj[0].resolution_class = buf["stats"].at(0), buf["means"].at(0), 1, 0
        dt = PN.DetectArrays(buf["dlcu"].ptr.value, buf["dpic"].ptr.value)
        ok(lib, lib.svt_amd_picture_detect_batch_launch(ctx, dj, 1, w, h, C.byref(dt)))
        self.noise_launch()
        sj = (SR.SboJob * 1)()
        sj[0].stats, sj[0].ref_stats, sj[0].chroma, sj[0].detect, sj[0].histogram = (buf["stats"].at(0), buf["stats"].at(sizes[L.BLOCK_STATS]), buf["means"].at(0),
                                                                                     buf["dlcu"].at(0), buf["hist"].at(0))
        for k in range(3):
            sj[0].zz[k] = buf["zz"].at(k * sizes[L.ZZ_SAD])
        sj[0].me, sj[0].ois, sj[0].cur_slot = None, None, 1
        sj[0].zz_count, sj[0].slice_type, sj[0].temporal_layer_index, sj[0].is_used_as_reference, sj[0].want_qpm = 3, 2, 3, 0, 1
        sbt = SR.SboArrays(buf["sbo_lcu"].ptr.value, buf["sbo_pic"].ptr.value)
        ok(lib, lib.svt_amd_source_ops_batch_launch(ctx, sj, 1, w, h, rw, rh, C.byref(sbt)))
        # the initial rate control: the picture's window is itself three times over, four frames to check
        io = self.irc_at = dict(checks=buf["irc"].at(0), motion=buf["irc"].at(_up(nl * 4)), lcu=buf["irc"].at(_up(nl * 4) + 256))
        io["stationary_edge"] = io["lcu"] + _up(nl * 48)
        io["pm_stationary_edge"] = io["stationary_edge"] + _up(64 * ((nl + 63) // 64))
        io["picture"] = io["pm_stationary_edge"] + _up(64 * ((nl + 63) // 64))
        lists = dict(look_ahead=1, frames_to_check=4, edge=[0], hom=[0, 0, 0], pan=[0])
        ij = (IM.IrcJob * 1)()
        ij[0].stats, ij[0].me, ij[0].cur_slot = buf["stats"].at(0), None, 1
        IM.fill_job(ij[0], dict(IR.pic(IR.B, 3), poc=0, eos=0), 0, lists,
                    lambda kind, k: {"stats": buf["stats"].at(0), "detect": buf["dlcu"].at(0)}.get(kind) or io[kind])
        it = IM.IrcArrays(*[io[k] for k in ("checks", "motion", "lcu", "stationary_edge", "pm_stationary_edge", "picture")])
        ok(lib, lib.svt_amd_initial_rc_batch_launch(ctx, ij, 1, w, h, C.byref(it)))
        dj2 = (MM.MdcJob * 1)()
        MM.fill_scalars(dj2[0], self.mjb, 261, [12171, 78934])
        dj2[0].me, dj2[0].cur_slot = None, 1
        dj2[0].stats, dj2[0].detect, dj2[0].sbo_lcu, dj2[0].sbo_pic = buf["stats"].at(0), buf["dlcu"].at(0), buf["sbo_lcu"].ptr.value, buf["sbo_pic"].ptr.value
        dj2[0].pic_detect, dj2[0].noise_pic, dj2[0].stationary_edge = buf["dpic"].ptr.value, buf["noise"].ptr.value, io["stationary_edge"]
        mt = MM.MdcArrays(buf["mdc_lcu"].ptr.value, buf["mdc_pic"].ptr.value)
        ok(lib, lib.svt_amd_md_config_batch_launch(ctx, dj2, 1, w, h, C.byref(mt)))
        # ... and this entry: every pointer is an array one of the launches above writes
        self.where = dict(mdc_lcu=buf["mdc_lcu"].ptr.value, stats=buf["stats"].at(0), detect=buf["dlcu"].at(0), sbo_lcu=buf["sbo_lcu"].ptr.value,
                          sbo_pic=buf["sbo_pic"].ptr.value, irc_lcu=io["lcu"], ac_energy=buf["energy"].at(0), stationary_edge=io["stationary_edge"], sticky=None)
        cjob = (M.MdCtlJob * 1)()
        M.fill_job(cjob[0], self.jb, lambda kind: self.where[kind])
        before = markers(lib, ctx)
        ok(lib, launch(lib, ctx, cjob, 1, w, h, self.controls.at()))
        self.marker_change = tuple(a - b for a, b in zip(markers(lib, ctx), before))

    def noise_launch(self):
        """the noise detection of slot 1: the picture record the configuration reads"""
        nj = (NZ.NoiseJob * 1)()
        nj[0].cur_slot, nj[0].method, nj[0].noise_detection_th = 1, 2, 0       # SVT_AMD_NOISE_FULL
        nt = NZ.NoiseArrays(self.buf["flat"].ptr.value, self.buf["noise"].ptr.value)
        ok(self.lib, self.lib.svt_amd_noise_detect_batch_launch(self.ctx, nj, 1, C.byref(nt)))

    def inputs(self):
        """the records the controls were made from, downloaded (the first wait of the chain)"""
        nl, buf = self.nl, self.buf
        irc = buf["irc"].get()
        base = buf["irc"].at(0)
        cut = lambda key, nbytes: irc[self.irc_at[key] - base:self.irc_at[key] - base + nbytes]  # noqa: E731
        return dict(mdc_lcu=buf["mdc_lcu"].get().view(MR.MDC_LCU_DTYPE), stats=buf["stats"].get().view(S.PA_LCU_STATS_DTYPE).reshape(3, nl)[0],
                    detect=buf["dlcu"].get().view(PN.LCU_DETECT_DTYPE), sbo_lcu=buf["sbo_lcu"].get().view(SR.SBO_LCU_DTYPE),
                    sbo_pic=buf["sbo_pic"].get().view(SR.SBO_PIC_DTYPE), irc_lcu=cut("lcu", nl * 48).view(IR.IRC_LCU_DTYPE),
                    ac_energy=buf["energy"].get().view("<u8").reshape(3, nl, 5)[0], stationary_edge=cut("stationary_edge", nl), sticky=None)

    def free(self):
        for b in list(self.buf.values()) + [self.controls]:
            b.free()
        self.lib.svt_amd_context_destroy(self.ctx)


def test_chain_on_one_lane_reads_the_records_where_they_lie(lib):
    """the controls equal the restatement run on the downloaded inputs, and the entry adds neither a completion marker nor a wait"""
    ch = Chain(lib, 71)
    try:
        assert ch.marker_change == (0, 0), ch.marker_change
        got = ch.controls.download()                                # the first wait of the chain
        rec = ch.inputs()
        assert rec["mdc_lcu"]["leaf_count"].any() and rec["ac_energy"].any() and rec["stats"]["variance"].any()
        same(got[0], N.md_controls(ch.W, ch.H, rec, ch.jb), "chain")
        for f in ("leaf_count", "leaf_index", "leaf_split"):
            assert np.array_equal(got[0][f], rec["mdc_lcu"][f]), f
    finally:
        ch.free()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_entry_and_queue_nothing(lib):
    name = "partial_416x240"
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    ctx = make_context(lib, w, h, 1)
    pics = case_pictures(lib, ctx, name)
    out = Out(lib, ctx, 2, w, h)
    ok(lib, lib.svt_amd_synchronize(ctx))
    before = markers(lib, ctx)

    def bad(change, what, i=0, **launch_args):
        pair = (M.MdCtlJob * 2)()
        pair[0], pair[1] = pics.job(2), pics.job(i)
        change(pair[1])
        args = dict(n=2, w=w, h=h, out=out.at())
        args.update(launch_args)
        refused(lib, launch(lib, ctx, pair, args["n"], args["w"], args["h"], args["out"]), M.ENTRY, what)
        assert b"job 1" in lib.svt_amd_last_error() or launch_args, lib.svt_amd_last_error()

    def setter(field, value):
        return lambda j: setattr(j, field, value)

    def pad(k):
        def change(j):
            j.pad[k] = 1
        return change

    try:
        assert jobs[0]["mdc"] and jobs[0]["irc"] and jobs[0]["depth_mode"] == 0 and not jobs[5]["mdc"]
        for field in ("stats", "detect", "sbo_lcu", "sbo_pic"):
            bad(setter(field, None), field)
        bad(setter("mdc_lcu", None), "no configuration records under depth mode 0")
        for mode in (0, 3, 4, 5):
            bad(setter("depth_mode", mode), "no configuration records under depth mode %d" % mode, i=5)
        bad(setter("irc_lcu", None), "energies without initial rate control records")
        bad(setter("ac_energy", None), "initial rate control records without energies")
        bad(setter("slice_type", 3), "slice type")
        bad(setter("chroma_level", 6), "chroma level")
        bad(setter("resolution_class", 4), "class")
        bad(setter("depth_mode", 6), "depth mode")
        bad(setter("tile_cols", 0), "no tile column")
        bad(setter("tile_rows", 0), "no tile row")
        bad(setter("tile_cols", 8), "more tile columns than LCU columns")
        bad(setter("tile_rows", 5), "more tile rows than LCU rows")
        bad(setter("pad0", 1), "pad0")
        for k in range(4):
            bad(pad(k), "pad[%d]" % k)
        bad(lambda j: None, "more than 16,384 LCUs", w=8256, h=8192)   # 129 x 128 = 16,512
        bad(lambda j: None, "larger than the context", w=w + 64)
        bad(lambda j: None, "no output array", out=None)
        for n in (0, -1, M.MAX_BATCH + 1):
            bad(lambda j: None, "job count", n=n)
        assert markers(lib, ctx) == before                          # no completion record, no wait
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert out.untouched()
        pair = (M.MdCtlJob * 2)()                                    # ... and the same pair, unchanged, runs
        pair[0], pair[1] = pics.job(2), pics.job(5)
        ok(lib, launch(lib, ctx, pair, 2, w, h, out.at()))
        same(out.download(), g["lcu"][[2, 5]], "after the refusals")
    finally:
        out.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 7. a batch of one and the largest batch -----------------------------------------------------------------------------------------------------------

def test_a_batch_of_one_and_the_largest_batch(lib):
    name = "one_64x64"
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    count = len(jobs)
    ctx = make_context(lib, w, h, 1)
    pics = case_pictures(lib, ctx, name)
    one, big = Out(lib, ctx, 1, w, h), Out(lib, ctx, M.MAX_BATCH, w, h)
    try:
        ok(lib, launch(lib, ctx, pics.job_array([2]), 1, w, h, one.at()))
        same(one.download(), g["lcu"][[2]], "a batch of one")
        order = [i % count for i in range(M.MAX_BATCH)]
        ok(lib, launch(lib, ctx, pics.job_array(order), M.MAX_BATCH, w, h, big.at()))
        same(big.download(), g["lcu"][order], "256")
    finally:
        for o in (one, big):
            o.free()
        pics.free()
        lib.svt_amd_context_destroy(ctx)


# ---- Part B: the mode-decision call reads a bound device array in place ---------------------------------------------------------------------------------

def _md_sig(lib):
    vp = C.c_void_p
    lib.svt_amd_md_encode_picture.restype = C.c_int
    lib.svt_amd_md_encode_picture.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_int, vp, vp, vp, vp]
    lib.svt_amd_md_encode_picture16.restype = C.c_int
    lib.svt_amd_md_encode_picture16.argtypes = lib.svt_amd_md_encode_picture.argtypes
    lib.svt_amd_md_encode_picture_inter.restype = C.c_int
    lib.svt_amd_md_encode_picture_inter.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_create.restype = C.c_int
    lib.svt_amd_encdec_picture_create.argtypes = [vp, C.c_uint16, C.c_uint16, C.c_int, C.POINTER(vp)]
    lib.svt_amd_encdec_picture_destroy.argtypes = [vp, vp]
    lib.svt_amd_encdec_picture_set_inter.restype = C.c_int
    lib.svt_amd_encdec_picture_set_inter.argtypes = [vp] * 5
    lib.svt_amd_md_lcus_supported.restype, lib.svt_amd_md_lcus_supported.argtypes = C.c_int, [vp, vp, C.c_int]


def decisions(md_out):
    """the bytes of an SvtAmdMdLcuOut array that the call DEFINES.  At the start of an LCU the kernel sets tested = 0 and split = 1 for all 85 leaves and nothing else
    (md_logic.h, md_construct_cu_array); at its end it copies every leaf's state out, so the other fields of a leaf the LCU never tested - and the inter fields of a
    tested leaf that is no inter / no merge unit - hold whatever the workgroup's LDS held: the previous LCU that workgroup drew a ticket for, or what an earlier
    kernel left on that CU.  They are no function of the call's inputs - two calls with the SAME host records differ in thousands of those bytes (measured:
    CHANGELOG round 25) - the header promises them "of tested leaves" / "(merge units)" only, and compare_md of the existing suite reads exactly the domains below.
    Everything else is compared byte for byte: split and tested of all leaves, the pad, the mode fields and the cost of every tested leaf, the vectors of every
    inter leaf, merge index and merge / skip cost of every merge leaf"""
    a = np.frombuffer(md_out, S.MD_LCU_OUT_DTYPE).copy()
    tested = a["tested"] == 1
    inter = tested & (a["pred_mode"] == 1)
    merge = inter & (a["merge_flag"] == 1)
    domain = dict(pred_mode=tested, intra_luma_mode=tested, ycbf=tested, cost=tested, inter_dir=tested, merge_flag=tested, mv=inter, merge_index=merge, merge_cost=merge,
                  skip_cost=merge)
    assert set(domain) | {"split", "tested", "pad"} == set(a.dtype.names)
    for f, keep in domain.items():
        a[f][~keep] = 0
    return a.tobytes()


def same_call(host, bound, tag):
    assert decisions(host[0]) == decisions(bound[0]), (tag, "md_out")
    assert host[1] == bound[1], (tag, "works")
    assert host[2] == bound[2], (tag, "results")


class Rect(C.Structure):
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("w", C.c_uint16), ("h", C.c_uint16)]


class MdWorld:
    """a context, a picture object and picture k of a mode-decision fixture; call(host, bound) -> rc and the three result arrays as bytes, each filled with
    SENTINEL before the call.  host: an array of records, or None; bound: an array of records that is copied to the device and bound, or None"""

    def __init__(self, lib, g, k=0, bps=1, P=None):
        import torch
        _md_sig(lib)
        self.lib, self.g, self.k, self.bps = lib, g, k, bps
        self.w, self.h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
        self.inter = "inter" in g.files
        self.ctx, self.pic = C.c_void_p(), C.c_void_p()
        ok(lib, lib.svt_amd_context_create(0, self.w, (self.h + 7) & ~7, 2, C.byref(self.ctx)))
        ok(lib, lib.svt_amd_encdec_picture_create(self.ctx, self.w, self.h, bps, C.byref(self.pic)))
        self.P = np.ascontiguousarray(g["pic"][k:k + 1]) if P is None else P
        self.cost, self.ois = np.ascontiguousarray(g["cost"][k]), np.ascontiguousarray(g["ois"][k])
        self.src = [np.ascontiguousarray(g[n][k]) for n in ("src_y", "src_cb", "src_cr")]
        if bps == 2:
            rng = np.random.default_rng(10)
            self.src = [((a.astype(np.uint16) << 2) | rng.integers(0, 4, a.shape, dtype=np.uint16)).astype(np.uint16) for a in self.src]
        self.lcus = np.ascontiguousarray(g["lcu"][k])
        self.n = len(self.lcus)
        self.dev = DeviceBuffer(lib, self.ctx, self.n * REC + 64)
        if self.inter:
            self.X, self.me, self.tmvp, refs, planes = inter_inputs(g, k)
            self.ref_dev = [[torch.from_numpy(a).cuda() for a in pl] for pl in planes]
            torch.cuda.synchronize()
            rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r.strideY, r.strideC, r.originX, r.originY, r.width, r.height)
                  for d, r in zip(self.ref_dev, refs)]
            ok(lib, lib.svt_amd_encdec_picture_set_inter(self.ctx, self.pic, C.byref(rs[0]), C.byref(rs[1]), self.cost.ctypes.data))

    def bind(self, records, offset=0):
        """the records into device memory on the context's lane (stream order is all the binding needs), and bound"""
        self.bound_keep = np.ascontiguousarray(records)
        self.dev.put(self.bound_keep, offset)
        ok(self.lib, self.lib.svt_amd_md_picture_set_controls(self.ctx, self.pic, C.c_void_p(self.dev.at(offset))))

    def call(self, host=None, bound=None, bind_ptr=None):
        lib, n = self.lib, self.n
        wide = self.bps == 2
        out = np.full(n, SENTINEL, np.uint8).repeat(S.MD_LCU_OUT_DTYPE.itemsize).view(S.MD_LCU_OUT_DTYPE)
        works = np.full(n * (S.LCU_WORK16_DTYPE if wide else S.LCU_WORK_DTYPE).itemsize, SENTINEL, np.uint8)
        res = np.full(n * (S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE).itemsize, SENTINEL, np.uint8)
        if bound is not None:
            self.bind(bound)
        if bind_ptr is not None:
            ok(lib, lib.svt_amd_md_picture_set_controls(self.ctx, self.pic, C.c_void_p(bind_ptr)))
        hp = np.ascontiguousarray(host).ctypes.data if host is not None else None
        s = self.src
        if self.inter:
            rc = lib.svt_amd_md_encode_picture_inter(self.ctx, self.pic, self.P.ctypes.data, self.X.ctypes.data, hp, s[0].ctypes.data, s[0].shape[1], s[1].ctypes.data,
                                                     s[2].ctypes.data, s[1].shape[1], self.ois.ctypes.data, 0, self.me.ctypes.data, 0,
                                                     self.tmvp.ctypes.data if self.tmvp is not None else None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        else:
            fn = lib.svt_amd_md_encode_picture16 if wide else lib.svt_amd_md_encode_picture
            rc = fn(self.ctx, self.pic, self.P.ctypes.data, hp, s[0].ctypes.data, s[0].shape[1], s[1].ctypes.data, s[2].ctypes.data, s[1].shape[1],
                    self.ois.ctypes.data, 0, self.cost.ctypes.data, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        return rc, (out.tobytes(), works.tobytes(), res.tobytes())

    def free(self):
        self.dev.free()
        self.lib.svt_amd_encdec_picture_destroy(self.ctx, self.pic)
        self.lib.svt_amd_context_destroy(self.ctx)


def _host_and_bound_agree(lib, name, bps=1):
    g = np.load(os.path.join(S.GOLDEN_DIR, "md_%s.npz" % name))
    for k in range(min(2, len(g["picture_number"]))):
        world = MdWorld(lib, g, k, bps)
        try:
            rc, host = world.call(host=world.lcus)
            assert rc == 0, lib.svt_amd_last_error()
            rc, bound = world.call(bound=world.lcus)
            assert rc == 0, lib.svt_amd_last_error()
            same_call(host, bound, (name, k))
            assert not is_sentinel(np.frombuffer(host[0], np.uint8))
            # the summary the call took of the bound array
            chk = np.zeros((), R.CHECK_DTYPE)
            ok(lib, lib.svt_amd_debug_md_controls_check(world.ctx, C.c_void_p(world.dev.at(0)), world.n, int(world.P["depth_mode"][0]), int(world.inter), chk.ctypes.data))
            assert chk.tobytes() == N.check_summary(world.lcus, int(world.P["depth_mode"][0]), world.inter).tobytes(), (name, k)
            assert int(chk["first_bad"]) == 0xFFFFFFFF
        finally:
            world.free()


@pytest.mark.parametrize("name", ["b_motion_416x240_m8", "bref_motion_416x240_m8", "b_tiles_motion_640x384_m8"])
def test_p_and_b_pictures_decide_the_same_from_a_bound_device_array(lib, name):
    """8. svt_amd_md_encode_picture_inter once with the fixture's host records, once with the same records in device memory and bound: byte-identical
    decisions, work records and results.  The tiles fixture gives the call its tile count (4) through the check record"""
    _host_and_bound_agree(lib, name)


@pytest.mark.parametrize("name,bps", [("i_motion_416x240_m9", 1), ("i_motion_416x240_m9", 2)])
def test_i_pictures_and_ten_bits_decide_the_same_from_a_bound_device_array(lib, name, bps):
    """9. the same through svt_amd_md_encode_picture and svt_amd_md_encode_picture16"""
    _host_and_bound_agree(lib, name, bps)


def test_controls_made_on_the_device_and_bound_decide_as_the_same_records_from_the_host(lib):
    """10. end to end: the controls of the chain, produced on the device, bound from ANOTHER context's array (the chain's lane is synchronised first: ordering a
    foreign array is the caller's), against the same records downloaded and passed as host memory - the picture, source and records of a recorded B picture.
    A chain whose records the host path does not cover (svt_amd_md_lcus_supported) is passed over; at least one must run"""
    g = np.load(os.path.join(S.GOLDEN_DIR, "md_b_xc_whiteblack_192x128_m8_q0.npz"))
    ran = 0
    for seed in (71, 73, 79, 83, 89, 97):
        ch = Chain(lib, seed, chroma_level=int(g["pic"][0]["chroma_level"]), depth_mode=int(g["pic"][0]["depth_mode"]))
        world = MdWorld(lib, g, 0)
        try:
            assert (world.w, world.h) == (ch.W, ch.H)
            records = np.ascontiguousarray(ch.controls.download()[0])          # waits for the chain's lane
            if lib.svt_amd_md_lcus_supported(world.P.ctypes.data, records.ctypes.data, len(records)) != 1 or not (records["leaf_count"] > 0).all():
                continue
            rc, host = world.call(host=records)
            assert rc == 0, lib.svt_amd_last_error()
            rc, bound = world.call(bind_ptr=ch.controls.at())
            assert rc == 0, lib.svt_amd_last_error()
            same_call(host, bound, seed)
            ran += 1
            break
        finally:
            world.free()
            ch.free()
    assert ran >= 1


def test_refused_mode_decision_calls_leave_everything_as_it_was(lib):
    """11. every refusal around a binding; md_out keeps its sentinel, the error names the entry and the LCU, and a further call with host records gives the
    fixture's decisions again"""
    g = np.load(os.path.join(S.GOLDEN_DIR, "md_b_motion_416x240_m8.npz"))
    world = MdWorld(lib, g, 0)
    lib.svt_amd_encdec_picture_set_rect.restype, lib.svt_amd_encdec_picture_set_rect.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]
    try:
        assert int(world.P["depth_mode"][0]) == 0
        rc, want = world.call(host=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()

        def still_works(tag):
            rc, got = world.call(host=world.lcus)
            assert rc == 0, (tag, lib.svt_amd_last_error())
            same_call(want, got, tag)

        def refusal(tag, lcu=None, text=None, **call):
            rc, got = world.call(**call)
            assert rc == BAD_PARAM, (tag, rc)
            assert all(is_sentinel(np.frombuffer(a, np.uint8)) for a in got), tag
            err = lib.svt_amd_last_error()
            if lcu is not None:
                assert err.startswith(b"svt_amd_md_encode_picture") and (b"LCU %d" % lcu) in err, (tag, err)
            if text is not None:
                assert err.startswith(b"svt_amd_md_encode_picture") and text in err, (tag, err)
            still_works(tag)

        def changed(i, **fields):
            records = world.lcus.copy()
            for f, v in fields.items():
                records[f][i] = v
            return records

        refusal("NULL without a binding")
        rc, _ = world.call(bound=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()
        refusal("a second NULL call after the binding was consumed")
        refusal("host records together with a binding", text=b"bound", host=world.lcus, bound=world.lcus)
        refusal("... which dropped the binding")
        refusal("leaf_count 0", lcu=9, bound=changed(9, leaf_count=0))
        descending = world.lcus.copy()
        i = int(np.flatnonzero(descending["leaf_count"] >= 2)[-1])
        descending["leaf_index"][i, :2] = descending["leaf_index"][i, :2][::-1].copy()
        refusal("a descending leaf pair", lcu=i, text=b"not ascending", bound=descending)
        refusal("lcu_md_mode 3 under depth mode 0", lcu=4, text=b"svt_amd_md_encode_picture_inter", bound=changed(4, lcu_md_mode=3))
        refusal("chroma_encode_mode 0", lcu=27, text=b"svt_amd_md_encode_picture_inter", bound=changed(27, chroma_encode_mode=0))
        two = changed(20, leaf_count=0)
        two["chroma_encode_mode"][3] = 0
        refusal("the first offender is named", lcu=3, bound=two)
        rect = Rect(0, 0, 192, 128)
        ok(lib, lib.svt_amd_encdec_picture_set_rect(world.ctx, world.pic, C.byref(rect)))
        rc, got = world.call(bound=world.lcus)
        assert rc == BAD_PARAM and b"rectangle" in lib.svt_amd_last_error() and lib.svt_amd_last_error().startswith(b"svt_amd_md_encode_picture")
        assert all(is_sentinel(np.frombuffer(a, np.uint8)) for a in got)
        ok(lib, lib.svt_amd_encdec_picture_set_rect(world.ctx, world.pic, None))
        still_works("after the rank rectangle")
        refusal("... and that call consumed its binding too")
    finally:
        world.free()
