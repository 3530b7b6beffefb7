"""The batched scene-transition detection on the device (include/svt_hevc_amd.h "Batched scene-transition detection"; svt-hevc_amd/csrc/scd_kernels.hip) through the
C-ABI: svt_amd_scene_detect_batch_launch on the planted cases of tests/scd_records.py against the restatement (tests/scd_numpy.py) byte for byte and against
what the REFERENCE's own function left (tests/golden/scd_*.npz); one batch against the same jobs in batches queued back to back, each resuming from the state
the one before left on the device; queued behind the side statistics, the chroma statistics and the detectors on one lane, reading their arrays where they
lie; sentinel outputs; refusals."""
import ctypes as C

import numpy as np
import pytest

import pa_detect_numpy as PN
import scd_numpy as N
import scd_records as R
import scdlib as M
import sidelib as L
from gpu_util import upload
from pa_batch_util import DeviceBuffer, is_sentinel, make_context, markers, ok, refused, round_up as _up
from test_oracle_pa import oracle_picture as pa_oracle

pytestmark = pytest.mark.gpu
CASES = list(R.CASES)
KINDS = ("picture", "ahd", "state")
SIZES = dict(picture=R.PIC_DTYPE.itemsize, ahd=16 * 3 * 4, state=R.STATE_DTYPE.itemsize)


@pytest.fixture(scope="module")
def lib(product):
    return M.declare(product)


@pytest.fixture(scope="module")
def ctx(lib):
    """a context made for ONE LCU: the entry reads no picture slot, so no case has to fit it"""
    c = make_context(lib, 64, 64, 1)
    yield c
    lib.svt_amd_context_destroy(c)


class Outputs:
    """the three output arrays for n jobs, filled with SENTINEL"""

    def __init__(self, lib, ctx, n):
        self.lib, self.n = lib, n
        assert [SIZES[k] for k in KINDS] == [lib.svt_amd_scene_detect_bytes(which, 4, 4) for which in range(3)]
        self.buf = {k: DeviceBuffer(lib, ctx, n * SIZES[k]) for k in KINDS}

    def table(self, first=0):
        """the table of a batch whose job 0 lands at place `first` of the arrays"""
        return M.ScdArrays(*[self.buf[k].at(first * SIZES[k]) for k in KINDS])

    def state_at(self, place):
        return self.buf["state"].at(place * SIZES["state"])

    def raw(self):
        return {k: self.buf[k].get().reshape(self.n, -1) for k in KINDS}

    def download(self, first=0, count=None):
        raw = self.raw()
        last = self.n if count is None else first + count
        return dict(picture=raw["picture"][first:last].copy().view(R.PIC_DTYPE)[:, 0], ahd=raw["ahd"][first:last].copy().view(R.AHD_DTYPE).reshape(-1, 16, 3),
                    state=raw["state"][first:last].copy().view(R.STATE_DTYPE)[:, 0])

    def untouched(self):
        return all(is_sentinel(b.get()) for b in self.buf.values())

    def free(self):
        for b in self.buf.values():
            b.free()


class Records:
    """the records of the pictures of a case in device memory, and the jobs that point at them"""
    PARTS = ("luma", "chroma", "avg", "detect")

    def __init__(self, lib, ctx, pictures):
        self.keep, self.where = [], []
        self.dev = DeviceBuffer(lib, ctx, sum(_up(p[k].nbytes) for p in pictures for k in self.PARTS))
        off = 0
        for p in pictures:
            at = {}
            for k in self.PARTS:
                a = np.ascontiguousarray(p[k])
                self.keep.append(a)
                self.dev.put(a, off)
                at[k], off = self.dev.at(off), off + _up(a.nbytes)
            self.where.append(at)

    def jobs(self, first, count):
        """jobs first .. first + count - 1 of the case: job i is the call for picture i + 1"""
        jobs = (M.ScdJob * count)()
        for k in range(count):
            past, cur, future = self.where[first + k], self.where[first + k + 1], self.where[first + k + 2]
            j = jobs[k]
            j.past_histogram, j.cur_histogram, j.past_chroma_histogram, j.cur_chroma_histogram = past["luma"], cur["luma"], past["chroma"], cur["chroma"]
            j.past_region_average, j.cur_region_average, j.future_region_average = past["avg"], cur["avg"], future["avg"]
            j.past_detect, j.cur_detect = past["detect"], cur["detect"]
        return jobs

    def free(self):
        self.dev.free()


def launch(lib, ctx, jobs, n, geometry, state_in, table):
    w, h, rw, rh, mode = geometry
    return lib.svt_amd_scene_detect_batch_launch(ctx, jobs, n, w, h, rw, rh, mode, state_in, C.byref(table))


# ---- 1. every case against the restatement and the reference's record ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_every_case_gives_the_restatements_bytes_and_the_references_results(lib, ctx, name):
    geometry, jobs = R.CASES[name][:5], R.CASES[name][5]
    rec = Records(lib, ctx, R.case_pictures(name))
    out = Outputs(lib, ctx, jobs)
    try:
        t = out.table()
        ok(lib, launch(lib, ctx, rec.jobs(0, jobs), jobs, geometry, None, t))
        got = out.download()
        R.same(got, N.restated(name), name)                          # pads and the entries beyond the regions included
        N.same_as_reference(got, R.load_case(name), name)
    finally:
        out.free()
        rec.free()


# ---- 2. one batch against batches that resume from the state on the device ------------------------------------------------------------------------------

def test_split_batches_back_to_back_resume_from_the_state_on_the_device(lib, ctx):
    name = "long_256"
    geometry, jobs = R.CASES[name][:5], R.CASES[name][5]
    rec = Records(lib, ctx, R.case_pictures(name))
    whole, parts = Outputs(lib, ctx, jobs), Outputs(lib, ctx, jobs)
    try:
        t = whole.table()
        ok(lib, launch(lib, ctx, rec.jobs(0, jobs), jobs, geometry, None, t))
        first, keep = 0, []
        for count in (1, 2, 63, 190):                                # queued back to back on the one lane: nothing is waited for in between
            keep.append((rec.jobs(first, count), parts.table(first)))
            ok(lib, launch(lib, ctx, keep[-1][0], count, geometry, parts.state_at(first - 1) if first else None, keep[-1][1]))
            first += count
        assert first == jobs
        a, b = whole.raw(), parts.raw()
        for k in KINDS:
            assert a[k].tobytes() == b[k].tobytes(), k
        R.same(parts.download(), N.restated(name), name)
    finally:
        whole.free()
        parts.free()
        rec.free()


def test_a_state_given_on_the_device_is_the_constructors_state_when_it_says_so(lib, ctx):
    """d_state_in = the constructor's state equals NULL; any non-zero flag byte is a set flag"""
    name = "cut_512x320"
    geometry, jobs = R.CASES[name][:5], R.CASES[name][5]
    rec = Records(lib, ctx, R.case_pictures(name))
    out = Outputs(lib, ctx, jobs)
    state = R.constructor_state()
    state["reset_running_avg"] = 0x80
    dev = DeviceBuffer(lib, ctx, state.nbytes)
    try:
        dev.put(state)
        t = out.table()
        ok(lib, launch(lib, ctx, rec.jobs(0, jobs), jobs, geometry, dev.ptr, t))
        R.same(out.download(), N.restated(name), name)
    finally:
        dev.free()
        out.free()
        rec.free()


# ---- 3. in place behind the producers -------------------------------------------------------------------------------------------------------------------

def _texture(w, h, which, t):
    """(luma, cb, cr) of picture t of texture `which`: one seeded texture per `which`, a few samples of it moved by one from picture to picture"""
    rng, step = np.random.default_rng(900 + which), np.random.default_rng(950 + 10 * which + t)
    base = (70, 100, 150) if which == 0 else (170, 160, 90)
    planes = []
    for mean, shape in zip(base, ((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        p = mean + rng.integers(-14, 15, shape)
        flat = p.reshape(-1)
        flat[step.integers(0, flat.size, 48)] += 1
        planes.append(np.ascontiguousarray(p.astype(np.uint8)))
    return planes


def test_in_place_behind_side_statistics_chroma_statistics_and_detectors(lib, oracle):
    w, h, rw, rh, n = 512, 320, 4, 4, 8
    nl, plane = (w // 64) * (h // 64), (w // 2) * (h // 2)
    PN.declare(L.declare(lib))
    ctx = make_context(lib, w, h, n)
    frames = [_texture(w, h, t // 4, t) for t in range(n)]
    # the restatement on the numpy statistics: what the three producers are tested against
    pictures = []
    for luma, cb, cr in frames:
        stats, hist, ravg, _ = pa_oracle(oracle, np.ascontiguousarray(np.pad(luma, ((0, 64), (0, 64)), mode="edge")), w, h)
        chroma, _, _ = PN.chroma_histograms(cb, cr, w, h, rw, rh)
        _, pic = PN.detect(stats["variance"], stats["y_mean"], None, w, h, 0, 0)
        row = np.zeros(64, np.uint8)
        row[:16] = ravg.reshape(16)
        pictures.append(dict(luma=hist.reshape(16, 256), chroma=chroma.reshape(16, 2, 256), avg=row, detect=np.array([pic], PN.PIC_DETECT_DTYPE)))
    want = N.scene_detect(w, h, rw, rh, 1, [R.window(pictures, i) for i in range(n - 2)])
    assert want["picture"]["scene_change"].tolist() == [0, 0, 0, 1, 0, 0]      # picture 4 of pictures 1..6
    assert (want["picture"]["region_class"][3] == R.SCENE).all() and want["picture"]["reset_running_avg"].tolist() == [0, 0, 0, 1, 0, 0]
    for i in (0, 1, 2, 4, 5):                                                   # plane means more than 5 apart, histograms nearly disjoint
        assert want["ahd"][i].max() < want["ahd"][3].min() // 8
    assert abs(int(pictures[4]["avg"][0]) - int(pictures[3]["avg"][0])) > 5

    side = L.DeviceArrays(lib, ctx, n, w, h, rw, rh, absent=("ac_energy", "zz"))
    csz, dsz = PN.chroma_sizes(w, h, rw, rh), PN.detect_sizes(w, h)
    buf = dict(planes=DeviceBuffer(lib, ctx, n * 2 * plane), chist=DeviceBuffer(lib, ctx, n * csz[1]), cavg=DeviceBuffer(lib, ctx, n * csz[2]),
               csum=DeviceBuffer(lib, ctx, n * csz[3]), dlcu=DeviceBuffer(lib, ctx, n * dsz[0]), dpic=DeviceBuffer(lib, ctx, n * dsz[1]))
    out = Outputs(lib, ctx, n - 2)
    try:
        for i, (luma, cb, cr) in enumerate(frames):
            upload(lib, ctx, i, luma)
            buf["planes"].put(cb, 2 * i * plane), buf["planes"].put(cr, (2 * i + 1) * plane)
        ok(lib, L.launch(lib, ctx, L.make_jobs([(i, -1, 1, 0, 1) for i in range(n)]), side, rw, rh))
        cj, dj = (PN.ChromaJob * n)(), (PN.DetectJob * n)()
        for i in range(n):
            cj[i].cb, cj[i].cr, cj[i].pitch, cj[i].want_means, cj[i].want_histogram = buf["planes"].at(2 * i * plane), buf["planes"].at((2 * i + 1) * plane), w // 2, 0, 1
            dj[i].stats, dj[i].chroma, dj[i].want_edge16, dj[i].resolution_class = side.buf[L.BLOCK_STATS].at(i * side.sizes[L.BLOCK_STATS]), None, 0, 0
        ct = PN.ChromaArrays(None, buf["chist"].ptr.value, buf["cavg"].ptr.value, buf["csum"].ptr.value)
        ok(lib, lib.svt_amd_chroma_stats_batch_launch(ctx, cj, n, w, h, rw, rh, C.byref(ct)))
        dt = PN.DetectArrays(buf["dlcu"].ptr.value, buf["dpic"].ptr.value)
        ok(lib, lib.svt_amd_picture_detect_batch_launch(ctx, dj, n, w, h, C.byref(dt)))
        jobs = (M.ScdJob * (n - 2))()
        hist_at = lambda i: side.buf[L.HISTOGRAM].at(i * side.sizes[L.HISTOGRAM])          # noqa: E731
        avg_at = lambda i: side.buf[L.REGION_AVG].at(i * side.sizes[L.REGION_AVG])         # noqa: E731
        for k, j in enumerate(jobs):                                                       # the call for picture k + 1
            j.past_histogram, j.cur_histogram = hist_at(k), hist_at(k + 1)
            j.past_chroma_histogram, j.cur_chroma_histogram = buf["chist"].at(k * csz[1]), buf["chist"].at((k + 1) * csz[1])
            j.past_region_average, j.cur_region_average, j.future_region_average = avg_at(k), avg_at(k + 1), avg_at(k + 2)
            j.past_detect, j.cur_detect = buf["dpic"].at(k * dsz[1]), buf["dpic"].at((k + 1) * dsz[1])
        before = markers(lib, ctx)
        t = out.table()
        ok(lib, launch(lib, ctx, jobs, n - 2, (w, h, rw, rh, 1), None, t))
        assert markers(lib, ctx) == before                                                 # no completion record, no wait: stream order is all there is
        R.same(out.download(), want, "in place")                                           # the one synchronisation
    finally:
        for b in list(buf.values()) + [side, out]:
            b.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 4. sentinel outputs ----------------------------------------------------------------------------------------------------------------------------------

def test_a_batch_rewrites_every_byte_of_its_part_and_nothing_else(lib, ctx):
    name = "ragged_536x344_r3"                                       # nine regions: seven entries of every [16] are written as 0
    geometry, jobs = R.CASES[name][:5], R.CASES[name][5]
    rec = Records(lib, ctx, R.case_pictures(name))
    out = Outputs(lib, ctx, jobs + 3)
    try:
        t = out.table(2)
        ok(lib, launch(lib, ctx, rec.jobs(0, jobs), jobs, geometry, None, t))
        raw = out.raw()
        for k in KINDS:
            assert is_sentinel(raw[k][:2]) and is_sentinel(raw[k][2 + jobs:]), k
        got, want = out.download(2, jobs), N.restated(name)
        R.same(got, want, name)
        assert not got["picture"]["pad"].any() and not got["state"]["pad"].any() and not got["ahd"][:, 9:].any() and not got["picture"]["region_class"][:, 9:].any()
        assert not got["state"]["ahd_running_avg"][:, 9:].any() and not got["state"]["ahd_running_avg_cb"][:, 9:].any() and not got["state"]["ahd_running_avg_cr"][:, 9:].any()
    finally:
        out.free()
        rec.free()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_entry_and_queue_nothing(lib, ctx):
    name = "cut_512x320"
    geometry, jobs = R.CASES[name][:5], R.CASES[name][5]
    w, h, rw, rh, mode = geometry
    rec = Records(lib, ctx, R.case_pictures(name))
    out = Outputs(lib, ctx, jobs)
    t = out.table()
    ok(lib, lib.svt_amd_synchronize(ctx))
    before = markers(lib, ctx)

    def bad(what, change=None, n=2, table=t, job=None, **geo):
        pair = rec.jobs(0, 2)
        if change:
            setattr(pair[1], change, None)
        g = dict(w=w, h=h, rw=rw, rh=rh, mode=mode)
        g.update(geo)
        refused(lib, launch(lib, ctx, pair, n, (g["w"], g["h"], g["rw"], g["rh"], g["mode"]), None, table), M.ENTRY, what)
        if job is not None:
            assert b"job %d" % job in lib.svt_amd_last_error(), lib.svt_amd_last_error()
        elif n == 2 and what != "more than 16,384 LCUs":               # what belongs to the whole batch names no job
            assert b"job" not in lib.svt_amd_last_error(), lib.svt_amd_last_error()

    def table_without(kind):
        ptrs = [out.buf[k].ptr.value for k in KINDS]
        ptrs[KINDS.index(kind)] = None
        return M.ScdArrays(*ptrs)

    try:
        for field in M.JOB_FIELDS:
            bad("a NULL " + field, change=field, job=1)
            assert field.encode() in lib.svt_amd_last_error()
        for kind in KINDS:
            bad("no %s array" % kind, table=table_without(kind))
        for n in (0, -1, M.MAX_BATCH + 1):
            bad("job count", n=n)
        for regions in (dict(rw=0), dict(rw=5), dict(rh=0), dict(rh=5)):
            bad("regions", **regions)
        for m in (0, 3):
            bad("scd_mode", mode=m)
        bad("a width of 0", w=0)
        bad("a height of 4", h=4)
        bad("more than 16,384 LCUs", w=8256, h=8192)                   # 129 x 128 = 16,512
        assert markers(lib, ctx) == before                              # no completion record, no wait
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert out.untouched()
        ok(lib, launch(lib, ctx, rec.jobs(0, jobs), jobs, geometry, None, t))
        R.same(out.download(), N.restated(name), "a correct batch afterwards")
    finally:
        out.free()
        rec.free()
