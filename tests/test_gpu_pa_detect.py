"""-m gpu: the batched chroma statistics and picture detectors (svt_amd_chroma_stats_batch_launch, svt_amd_picture_detect_batch_launch;
svt-hevc_amd/csrc/detect_kernels.hip) behind svt_amd_side_stats_batch_launch on ONE lane - (1) against what the REFERENCE's GatheringPictureStatistics computed
(tests/golden/padetect_*.npz), (2) seeded variants against the numpy restatement that the CPU suite pins on those fixtures (tests/pa_detect_numpy.py),
(3) the detectors alone on synthetic statistics at the extremes, (4) per-picture selection, (5) two batches back to back, (6) the parameter checks.
Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import pa_detect_numpy as N
import pa_detect_pictures as P
import sidelib as L
import svtlib as S
from gpu_util import upload
from pa_batch_util import SENTINEL, DeviceBuffer, is_sentinel as _sentinel, make_context, ok as _ok, refused as _refused
from test_oracle_pa import oracle_picture as pa_oracle
from test_pa_detect_cpu import CASES, load_case

pytestmark = pytest.mark.gpu
CHROMA, DETECT = "svt_amd_chroma_stats_batch_launch", "svt_amd_picture_detect_batch_launch"
KINDS4 = ("objects", "noise", "motion", "static")


@pytest.fixture(scope="module")
def lib(product):
    return N.declare(L.declare(product))


def _context(lib, w, h, slots):
    return make_context(lib, max(w, 64), max(h, 64), slots)


class Batch:
    """the device arrays of an n-picture batch of both entries (+ the block statistics and the chroma planes they read)"""
    NAMES = ("stats", "means", "histogram", "region_average", "sum_chroma", "lcu", "picture", "planes")

    def __init__(self, lib, ctx, n, w, h, rw=4, rh=4):
        self.lib, self.ctx, self.n, self.w, self.h, self.rw, self.rh = lib, ctx, n, w, h, rw, rh
        self.nl, self.plane = S.lcu_count(w, h), (w // 2) * (h // 2)
        self.size = dict(zip(self.NAMES, [self.nl * 256] + N.chroma_sizes(w, h, rw, rh) + N.detect_sizes(w, h) + [2 * self.plane]))
        self.buf = {k: DeviceBuffer(lib, ctx, n * b) for k, b in self.size.items()}
        self.keep = []

    def put_chroma(self, i, cb, cr):
        cb, cr = np.ascontiguousarray(cb), np.ascontiguousarray(cr)
        self.keep += [cb, cr]
        self.buf["planes"].put(cb, i * 2 * self.plane), self.buf["planes"].put(cr, (i * 2 + 1) * self.plane)

    def side_stats(self, slots):
        """the block statistics of slot i into stats[i]: svt_amd_side_stats_batch_launch on the same lane"""
        jobs = L.make_jobs([(s, -1, 1, 0, 0) for s in slots])
        t = L.SideArrays(block_stats=self.buf["stats"].ptr.value)
        _ok(self.lib, self.lib.svt_amd_side_stats_batch_launch(self.ctx, jobs, len(jobs), 4, 4, C.byref(t)))

    def chroma_jobs(self, wants):
        """wants: (want_means, want_histogram) per picture; planes of picture i at planes[i]"""
        jobs = (N.ChromaJob * len(wants))()
        for i, (j, (m, hi)) in enumerate(zip(jobs, wants)):
            j.cb, j.cr, j.pitch, j.want_means, j.want_histogram = self.buf["planes"].at(i * 2 * self.plane), self.buf["planes"].at((i * 2 + 1) * self.plane), self.w // 2, m, hi
        return jobs

    def chroma_table(self):
        return N.ChromaArrays(*[self.buf[k].ptr.value for k in ("means", "histogram", "region_average", "sum_chroma")])

    def chroma(self, wants, table=None):
        jobs = self.chroma_jobs(wants)
        t = table or self.chroma_table()
        return self.lib.svt_amd_chroma_stats_batch_launch(self.ctx, jobs, len(jobs), self.w, self.h, self.rw, self.rh, C.byref(t))

    def detect_jobs(self, specs):
        """specs: (want_edge16, resolution class, with chroma means) per picture"""
        jobs = (N.DetectJob * len(specs))()
        for i, (j, (e, cls, with_chroma)) in enumerate(zip(jobs, specs)):
            j.stats, j.want_edge16, j.resolution_class = self.buf["stats"].at(i * self.size["stats"]), e, cls
            j.chroma = self.buf["means"].at(i * self.size["means"]) if with_chroma else None
        return jobs

    def detect_table(self):
        return N.DetectArrays(self.buf["lcu"].ptr.value, self.buf["picture"].ptr.value)

    def detect(self, specs, table=None):
        jobs = self.detect_jobs(specs)
        t = table or self.detect_table()
        return self.lib.svt_amd_picture_detect_batch_launch(self.ctx, jobs, len(jobs), self.w, self.h, C.byref(t))

    def download(self):
        raw = {k: self.buf[k].get().reshape(self.n, -1) for k in self.NAMES if k != "planes"}
        return dict(stats=raw["stats"].view(S.PA_LCU_STATS_DTYPE).reshape(self.n, -1), means=raw["means"].view(N.LCU_CHROMA_DTYPE).reshape(self.n, -1),
                    histogram=raw["histogram"].view(np.uint32).reshape(self.n, self.rw, self.rh, 2, 256), region_average=raw["region_average"].reshape(self.n, 64, 2),
                    sum_chroma=raw["sum_chroma"].view(np.uint64).reshape(self.n, 2), lcu=raw["lcu"].view(N.LCU_DETECT_DTYPE).reshape(self.n, -1),
                    picture=raw["picture"].view(N.PIC_DETECT_DTYPE).reshape(self.n))

    def untouched(self, names):
        return all(bool((self.buf[k].get() == SENTINEL).all()) for k in names)

    def free(self):
        for b in self.buf.values():
            b.free()


def _three_calls(lib, ctx, batch, frames, edges, cls):
    """frames: (luma, cb, cr) per picture -> planes up, then side statistics, chroma statistics and detectors queued on the one lane, nothing waited for in between"""
    for i, (luma, cb, cr) in enumerate(frames):
        upload(lib, ctx, i, luma)
        batch.put_chroma(i, cb, cr)
    batch.side_stats(list(range(len(frames))))
    _ok(lib, batch.chroma([(1, 1)] * len(frames)))
    _ok(lib, batch.detect([(e, cls, 1) for e in edges]))


def _assert_equals_checker(got, i, luma_stats, cb, cr, w, h, rw, rh, edge, cls, what):
    """picture i of a batch against the numpy restatement; luma_stats: the block statistics the detectors read (PA_LCU_STATS_DTYPE[lcus])"""
    means = N.chroma_means(cb, cr, w, h)
    assert got["means"][i].tobytes() == means.tobytes(), (what, i, "means")
    hist, ravg, total = N.chroma_histograms(cb, cr, w, h, rw, rh)
    assert np.array_equal(got["histogram"][i], hist), (what, i, "histogram")
    assert np.array_equal(got["region_average"][i], ravg) and np.array_equal(got["sum_chroma"][i], total), (what, i, "averages")
    lcu, pic = N.detect(luma_stats["variance"], luma_stats["y_mean"], means, w, h, edge, cls)
    for f in lcu.dtype.names:
        assert np.array_equal(got["lcu"][i][f], lcu[f]), (what, i, f, np.argwhere(got["lcu"][i][f] != lcu[f])[:4].tolist())
    assert got["picture"][i].tobytes() == pic.tobytes(), (what, i, got["picture"][i], pic)
    return lcu, pic


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_one_batch_per_clip_gives_what_the_reference_computed(lib, name):
    g, kind, w, h, seed, rw, rh = load_case(name)
    pictures = [int(t) for t in g["picture_number"]]
    n = len(pictures)
    ctx = _context(lib, w, h, n)
    batch = None
    try:
        batch = Batch(lib, ctx, n, w, h, rw, rh)
        frames = [(P.gen_luma(kind, w, h, t, seed),) + P.gen_chroma(kind, w, h, t, seed) for t in pictures]
        _three_calls(lib, ctx, batch, frames, [int(e) for e in g["want_edge16"]], int(g["resolution_class"][0]))
        got = batch.download()                                                   # the first wait
        for i, t in enumerate(pictures):
            what = (name, t)
            assert np.array_equal(got["stats"][i]["variance"], g["variance"][i]) and np.array_equal(got["stats"][i]["y_mean"], g["y_mean"][i]), what
            assert np.array_equal(got["means"][i]["cb_mean"], g["cb_mean"][i]) and np.array_equal(got["means"][i]["cr_mean"], g["cr_mean"][i]), what
            assert not got["means"][i]["pad"].any() and not got["lcu"][i]["pad"].any() and not got["picture"][i]["pad"].any(), what
            assert np.array_equal(got["histogram"][i], g["histogram"][i]), what
            assert np.array_equal(got["region_average"][i][:rw * rh].reshape(rw, rh, 2), g["region_average"][i]) and not got["region_average"][i][rw * rh:].any(), what
            assert np.array_equal(got["sum_chroma"][i], g["sum_chroma"][i]), what
            for f in ("var_of_var_32x32", "edge_cu", "homogeneous", "edge_block_num", "isolated_high_intensity", "sharp_edge"):
                assert np.array_equal(got["lcu"][i][f], g[f][i]), what + (f, np.argwhere(got["lcu"][i][f] != g[f][i])[:4].tolist())
            for f in ("pic_avg_variance", "very_low_var_pic", "logo_pic", "lcu_block_percentage"):
                assert int(got["picture"][i][f]) == int(g[f][i]), what + (f,)
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 2. seeded variants against the numpy checker --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(192, 136), (416, 240)])
def test_seeded_kinds_match_the_checker(lib, w, h):
    """the four gen_luma kinds with seeded chroma in one batch, 3 x 5 regions, the 16x16 edge map on every other picture, both small resolution classes' maps"""
    n, rw, rh = 4, 3, 5
    ctx = _context(lib, w, h, n)
    batch = None
    try:
        batch = Batch(lib, ctx, n, w, h, rw, rh)
        frames = [(S.gen_luma(k, w, h, 3 + i, 20 + i),) + P.gen_chroma(k, w, h, 3 + i, 20 + i) for i, k in enumerate(KINDS4)]
        edges = [1, 0, 1, 1]
        _three_calls(lib, ctx, batch, frames, edges, 1 if w == 416 else 0)       # 416x240 with the 7 x 4 map: every LCU is a potentialLogoLcu
        got = batch.download()
        for i, (luma, cb, cr) in enumerate(frames):
            lcu, _ = _assert_equals_checker(got, i, got["stats"][i], cb, cr, w, h, rw, rh, edges[i], 1 if w == 416 else 0, (w, h, KINDS4[i]))
            assert bool(lcu["edge_cu"].any()) == bool(edges[i])
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)


@pytest.mark.parametrize("bright", [((4, 4), (6, 5)), ((6, 5), (4, 4), (5, 4))])
def test_islands_at_the_ends_of_the_margin(lib, bright):
    """the bright LCUs at the first and the last position the +-4 rule allows (11 x 10 LCUs: columns 4..6, rows 4..5)"""
    w, h = 704, 640
    ctx = _context(lib, w, h, 1)
    batch = None
    try:
        batch = Batch(lib, ctx, 1, w, h)
        luma = P.islands(w, h, 9, bright=bright, step=(9, 8))
        cb, cr = P.gen_chroma("islands", w, h, 0, 9)
        _three_calls(lib, ctx, batch, [(luma, cb, cr)], [1], 0)
        got = batch.download()
        lcu, _ = _assert_equals_checker(got, 0, got["stats"][0], cb, cr, w, h, 4, 4, 1, 0, bright)
        iso = lcu["isolated_high_intensity"].reshape(10, 11)
        assert iso[0, 0] == 1 and iso[5, 6] == 1 and iso[5, 7] == 0 and iso[9, 10] == 0 and lcu["sharp_edge"].sum() == 1
        assert np.array_equal(lcu["isolated_high_intensity"], N.detect_sequential(got["stats"][0]["variance"], got["stats"][0]["y_mean"], w, h))
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)


def test_a_picture_of_incomplete_lcus_only(lib, oracle):
    """56x56: one LCU, incomplete.  A picture slot takes no picture below 64x64, so the block statistics come from the CPU checker (oracle/svt_oracle_pa.c) as an array."""
    w, h = 56, 56
    ctx = _context(lib, w, h, 1)
    batch = None
    try:
        batch = Batch(lib, ctx, 1, w, h, 2, 2)
        luma = S.gen_luma("objects", w, h, 1, 5)
        cb, cr = P.gen_chroma("objects", w, h, 1, 5)
        stats, _, _, _ = pa_oracle(oracle, P.padded(luma), w, h)
        batch.buf["stats"].put(stats)
        batch.put_chroma(0, cb, cr)
        _ok(lib, batch.chroma([(1, 1)]))
        _ok(lib, batch.detect([(1, 0, 1)]))
        got = batch.download()
        _assert_equals_checker(got, 0, stats, cb, cr, w, h, 2, 2, 1, 0, "56x56")
        assert not got["means"][0].view(np.uint8).any()
        assert got["lcu"][0]["homogeneous"][0] == 1 and (got["lcu"][0]["var_of_var_32x32"] == np.uint64(N.ALL_ONES)).all() and got["lcu"][0]["edge_cu"][0] == 0
        assert got["picture"][0]["very_low_var_pic"] == 0 and got["picture"][0]["logo_pic"] == 0 and got["picture"][0]["lcu_block_percentage"] == 0
        assert got["picture"][0]["pic_avg_variance"] == stats["variance"][0][0]
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 3. the detectors alone on synthetic statistics ------------------------------------------------------------------------------------------

def _synthetic(rng, nl, kind):
    stats, chroma = np.zeros(nl, S.PA_LCU_STATS_DTYPE), np.zeros(nl, N.LCU_CHROMA_DTYPE)
    edge_values = np.array([0, 1, 4, 5, 6, 19, 20, 21, 199, 200, 201, 4095, 4096, 4097, 65534, 65535], np.uint16)
    if kind == "max":
        stats["variance"] = 65535
    elif kind == "zero":
        stats["variance"] = 0
    elif kind == "thresholds":
        stats["variance"] = rng.choice(edge_values, size=(nl, 85))
    else:                                                                          # one huge 8x8 variance among small ones: the largest variance of variances
        stats["variance"] = rng.integers(0, 64, size=(nl, 85))
        stats["variance"][:, 21 + rng.integers(0, 64)] = 65535
        stats["variance"][:, 0] = rng.choice(np.array([139, 140, 141, 4, 5, 200, 201], np.uint16), size=nl)
    stats["y_mean"] = rng.choice(np.array([0, 119, 120, 121, 179, 180, 181, 255], np.uint8), size=(nl, 85))
    stats["y_mean"][4 * 11 + 5, 0], stats["y_mean"][4 * 11 + 4, 0] = 181, 119        # LCU (5, 4) marks its 9x9 whatever the draw
    chroma["cb_mean"] = rng.integers(0, 256, size=(nl, 21))
    chroma["cr_mean"] = rng.choice(np.array([0, 255], np.uint8), size=(nl, 21))
    return stats, chroma


def test_detectors_alone_on_synthetic_statistics_at_the_extremes(lib):
    """no planes: variances at 0, 65535 and the thresholds +-1, means at 120 / 180 +-1 uploaded as arrays - the 64-bit sums (64 x 65535^2 needs 38 bits), the
    unsigned subtraction, the 16-bit picture average (65535 x 110 / 110) and the comparisons at their edges"""
    w, h, kinds = 704, 640, ("max", "zero", "thresholds", "spike")
    nl, n = 110, 4
    rng = np.random.default_rng(17)
    ctx = _context(lib, w, h, 1)
    batch = None
    try:
        batch = Batch(lib, ctx, n, w, h)
        inputs = [_synthetic(rng, nl, k) for k in kinds]
        for i, (stats, chroma) in enumerate(inputs):
            batch.buf["stats"].put(stats, i * batch.size["stats"]), batch.buf["means"].put(chroma, i * batch.size["means"])
        specs = [(1, 0, 1), (1, 3, 1), (1, 1, 1), (0, 2, 0)]
        _ok(lib, batch.detect(specs))
        got = batch.download()
        for i, (stats, chroma) in enumerate(inputs):
            lcu, pic = N.detect(stats["variance"], stats["y_mean"], chroma, w, h, specs[i][0], specs[i][1])
            for f in lcu.dtype.names:
                assert np.array_equal(got["lcu"][i][f], lcu[f]), (kinds[i], f, np.argwhere(got["lcu"][i][f] != lcu[f])[:4].tolist())
            assert got["picture"][i].tobytes() == pic.tobytes(), (kinds[i], got["picture"][i], pic)
        assert got["picture"][0]["pic_avg_variance"] == 65535 and not got["lcu"][0]["var_of_var_32x32"].any() and got["picture"][0]["lcu_block_percentage"] == 65
        assert got["picture"][1]["very_low_var_pic"] == 1 and got["picture"][1]["logo_pic"] == 1 and got["lcu"][1]["homogeneous"].all()
        assert got["lcu"][3]["var_of_var_32x32"].max() > np.uint64(1 << 27) and not got["lcu"][3]["homogeneous"].any() and not got["lcu"][3]["edge_cu"].any()
        assert got["lcu"][2]["isolated_high_intensity"].any() and got["lcu"][2]["edge_cu"].any()
        assert _sentinel(batch.buf["histogram"].get()) and _sentinel(batch.buf["sum_chroma"].get())     # the other entry's arrays
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 4. selection ----------------------------------------------------------------------------------------------------------------------------

def test_selection_per_picture(lib):
    w, h, n, rw, rh = 416, 240, 5, 4, 4
    ctx = _context(lib, w, h, n)
    batch = None
    try:
        batch = Batch(lib, ctx, n, w, h, rw, rh)
        frames = [(S.gen_luma(KINDS4[i % 4], w, h, i, 31),) + P.gen_chroma(KINDS4[i % 4], w, h, i, 31) for i in range(n)]
        for i, (luma, cb, cr) in enumerate(frames):
            upload(lib, ctx, i, luma)
            batch.put_chroma(i, cb, cr)
        batch.side_stats(list(range(n)))
        #        means histogram
        wants = [(1, 1), (1, 0), (0, 1), (0, 0), (1, 1)]
        #        edge16 class with-means
        specs = [(1, 0, 1), (0, 0, 1), (0, 0, 0), (0, 0, 0), (1, 0, 1)]
        jobs = batch.chroma_jobs(wants)
        jobs[3].cb = jobs[3].cr = None                                           # nothing wanted of picture 3: its planes need not exist
        t = batch.chroma_table()
        _ok(lib, lib.svt_amd_chroma_stats_batch_launch(ctx, jobs, n, w, h, rw, rh, C.byref(t)))
        _ok(lib, batch.detect(specs))
        got = batch.download()
        for i, (luma, cb, cr) in enumerate(frames):
            means = N.chroma_means(cb, cr, w, h)
            hist, ravg, total = N.chroma_histograms(cb, cr, w, h, rw, rh)
            assert got["means"][i].tobytes() == means.tobytes() if wants[i][0] else _sentinel(got["means"][i]), (i, "means")
            if wants[i][1]:
                assert np.array_equal(got["histogram"][i], hist) and np.array_equal(got["region_average"][i], ravg) and np.array_equal(got["sum_chroma"][i], total), i
            else:
                assert _sentinel(got["histogram"][i]) and _sentinel(got["region_average"][i]) and _sentinel(got["sum_chroma"][i]), (i, "histogram")
            lcu, pic = N.detect(got["stats"][i]["variance"], got["stats"][i]["y_mean"], means if specs[i][2] else None, w, h, specs[i][0], 0)
            assert got["lcu"][i].tobytes() == lcu.tobytes() and got["picture"][i].tobytes() == pic.tobytes(), (i, "detect")
            assert bool(lcu["edge_cu"].any()) == bool(specs[i][0])               # want_edge16 0: edge_cu 0, also where chroma means are given
        # the optional arrays of the chroma entry: histograms without averages and sums
        for k in ("histogram", "region_average", "sum_chroma", "means"):
            batch.buf[k].fill()
        t = batch.chroma_table()
        t.means = t.region_average = t.sum_chroma = None
        _ok(lib, batch.chroma([(0, 1)] * n, t))
        got = batch.download()
        for i, (luma, cb, cr) in enumerate(frames):
            assert np.array_equal(got["histogram"][i], N.chroma_histograms(cb, cr, w, h, rw, rh)[0]), i
        assert _sentinel(got["means"]) and _sentinel(got["region_average"]) and _sentinel(got["sum_chroma"])
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 5. two batches back to back -------------------------------------------------------------------------------------------------------------

def test_two_batches_back_to_back_on_one_lane(lib):
    """nothing waited for between the six calls: the second batch's descriptor tables and its zeroing of the reduction scratch must not reach the first one's kernels"""
    w, h, rw, rh = 704, 640, 4, 4
    ctx = _context(lib, w, h, 5)
    first = second = None
    try:
        first, second = Batch(lib, ctx, 3, w, h, rw, rh), Batch(lib, ctx, 2, w, h, rw, rh)
        fa = [(P.islands(w, h, 40 + i, bright=((4 + i, 4), (5, 5))),) + P.gen_chroma("islands", w, h, i, 40) for i in range(3)]
        fb = [(S.gen_luma(k, w, h, 2, 50),) + P.gen_chroma(k, w, h, 2, 50) for k in ("objects", "noise")]
        for i, (luma, cb, cr) in enumerate(fa + fb):
            upload(lib, ctx, i, luma)
            (first if i < 3 else second).put_chroma(i if i < 3 else i - 3, cb, cr)
        ea, eb = [1, 0, 1], [1, 1]
        first.side_stats([0, 1, 2])
        _ok(lib, first.chroma([(1, 1)] * 3))
        _ok(lib, first.detect([(e, 0, 1) for e in ea]))
        second.side_stats([3, 4])
        _ok(lib, second.chroma([(1, 1)] * 2))
        _ok(lib, second.detect([(e, 0, 1) for e in eb]))
        ga, gb = first.download(), second.download()                             # one wait
        for got, frames, edges in ((ga, fa, ea), (gb, fb, eb)):
            for i, (luma, cb, cr) in enumerate(frames):
                _assert_equals_checker(got, i, got["stats"][i], cb, cr, w, h, rw, rh, edges[i], 0, ("batch", len(frames)))
        assert ga["lcu"]["isolated_high_intensity"].any() and not gb["lcu"]["isolated_high_intensity"].any()
    finally:
        for b in (first, second):
            if b:
                b.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 6. parameter checks ---------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_job_and_queue_nothing(lib):
    w, h, n = 416, 240, 3
    ctx = _context(lib, w, h, n)
    batch = None
    try:
        batch = Batch(lib, ctx, n, w, h)
        outputs = ("means", "histogram", "region_average", "sum_chroma", "lcu", "picture")

        def refused(rc, job, entry):
            _refused(lib, rc, entry, job)
            assert ("job %d" % job).encode() in lib.svt_amd_last_error(), lib.svt_amd_last_error()

        everything, detect_all = [(1, 1)] * n, [(1, 0, 1)] * n
        # a null required array
        jobs = batch.chroma_jobs(everything)
        jobs[2].cr = None
        t = batch.chroma_table()
        refused(lib.svt_amd_chroma_stats_batch_launch(ctx, jobs, n, w, h, 4, 4, C.byref(t)), 2, CHROMA)
        t = batch.chroma_table()
        t.means = None
        refused(batch.chroma([(0, 1), (1, 1), (1, 1)], t), 1, CHROMA)
        t = batch.chroma_table()
        t.histogram = None
        refused(batch.chroma(everything, t), 0, CHROMA)
        jobs = batch.detect_jobs(detect_all)
        jobs[1].stats = None
        t = batch.detect_table()
        refused(lib.svt_amd_picture_detect_batch_launch(ctx, jobs, n, w, h, C.byref(t)), 1, DETECT)
        for missing in ("lcu", "picture"):
            t = batch.detect_table()
            setattr(t, missing, None)
            refused(batch.detect(detect_all, t), 0, DETECT)
        # the 16x16 edge map wanted without chroma means
        refused(batch.detect([(1, 0, 1), (0, 0, 0), (1, 0, 0)]), 2, DETECT)
        refused(batch.detect([(0, 0, 1), (0, 4, 1), (0, 0, 1)]), 1, DETECT)              # no such resolution class
        # regions that do not fit: more than 64, none, regions below 8 luma samples
        for rw, rh in ((9, 8), (0, 4), (4, 0), (64, 1), (1, 31)):
            jobs = batch.chroma_jobs([(1, 0), (1, 1), (1, 1)])
            t = batch.chroma_table()
            refused(lib.svt_amd_chroma_stats_batch_launch(ctx, jobs, n, w, h, rw, rh, C.byref(t)), 1, CHROMA)
        jobs = batch.chroma_jobs(everything)
        jobs[1].pitch = w // 2 - 1
        t = batch.chroma_table()
        refused(lib.svt_amd_chroma_stats_batch_launch(ctx, jobs, n, w, h, 4, 4, C.byref(t)), 1, CHROMA)
        # 0 and 257 jobs
        big_c, big_d = (N.ChromaJob * 257)(), (N.DetectJob * 257)()
        tc, td = batch.chroma_table(), batch.detect_table()
        for count in (0, 257):
            _refused(lib, lib.svt_amd_chroma_stats_batch_launch(ctx, big_c, count, w, h, 4, 4, C.byref(tc)), CHROMA, count)
            assert b"jobs" in lib.svt_amd_last_error()
            _refused(lib, lib.svt_amd_picture_detect_batch_launch(ctx, big_d, count, w, h, C.byref(td)), DETECT, count)
            assert b"jobs" in lib.svt_amd_last_error()
        _ok(lib, lib.svt_amd_synchronize(ctx))
        assert batch.untouched(outputs), "a refused batch wrote"
        # ... and a following complete batch on the same context is right
        frames = [(S.gen_luma("motion", w, h, i, 3),) + P.gen_chroma("motion", w, h, i, 3) for i in range(n)]
        _three_calls(lib, ctx, batch, frames, [1] * n, 0)
        got = batch.download()
        for i, (luma, cb, cr) in enumerate(frames):
            _assert_equals_checker(got, i, got["stats"][i], cb, cr, w, h, 4, 4, 1, 0, "after the refused batches")
    finally:
        if batch:
            batch.free()
        lib.svt_amd_context_destroy(ctx)
