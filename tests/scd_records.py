"""Records for the batched scene-transition detection (include/svt_hevc_amd.h "Batched scene-transition detection"): the numpy layouts of the three outputs and of
the state, the PLANTED cases, and the case file tools/scd_logic_check.c (and the driver of tests/golden/make_scd_golden.py) reads.

The detector reads records only, so a case is a script: every picture of it is built from the one before by events that are chosen so that an inequality of the
detector holds.  A region's histogram of a plane is a fixed seeded floor plus N = (w // rw) * (h // rh) samples in two bins of a bin pair: N - m in one, m in the
other.  A `step` moves dm samples between the two (the sum of absolute differences against the picture before is exactly 2 * dm); a `cut` takes another, disjoint
bin pair (the sum is 2 * N).  `light` moves the region's average-intensity byte.  A case of J jobs has J + 2 pictures: job i is the call for picture i + 1 with
picture i as the past and picture i + 2 as the future one.  Everything comes back from the seeds: the fixtures hold results only."""
import os

import numpy as np

MAX_REGIONS = 16
NONE, GRADUAL, FLASH, FADE, SCENE = range(5)
PIC_DTYPE = np.dtype([("scene_change", "u1"), ("reset_running_avg", "u1"), ("abrupt_regions", "u1"), ("scene_regions", "u1"), ("region_count_threshold", "u1"),
                      ("pad", "u1", 3), ("region_class", "u1", 16)])
STATE_DTYPE = np.dtype([("ahd_running_avg", "<u4", 16), ("ahd_running_avg_cb", "<u4", 16), ("ahd_running_avg_cr", "<u4", 16), ("reset_running_avg", "u1"),
                        ("pad", "u1", 3)])
AHD_DTYPE = np.dtype("<u4")        # [n][16][3]
PIC_DETECT_DTYPE = np.dtype([("pic_avg_variance", "<u2"), ("very_low_var_pic", "u1"), ("logo_pic", "u1"), ("lcu_block_percentage", "u1"), ("pad", "u1", 3)])
ALL = "all"


def constructor_state():
    """PictureDecisionContextCtor: every running average 0, the flag set"""
    s = np.zeros(1, STATE_DTYPE)
    s["reset_running_avg"] = 1
    return s


class Script:
    """the pictures of a case, built one after the other"""

    def __init__(self, w, h, rw, rh, seed):
        self.w, self.h, self.rw, self.rh, self.regions = w, h, rw, rh, rw * rh
        self.n = (w // rw) * (h // rh)
        self.rng = np.random.default_rng(seed)
        self.floor = self.rng.integers(0, 40, (self.regions, 3, 256)).astype(np.int64)
        self.pair = self.rng.integers(0, 16, (self.regions, 3))
        self.m = self.rng.integers(self.n // 4, 3 * self.n // 8 + 1, (self.regions, 3))
        self.avg = self.rng.integers(60, 180, self.regions)
        self.var = 600
        self.pictures = []

    def _regions(self, which):
        return range(self.regions) if which is ALL else which

    def step(self, which, plane, dm):
        """2 * dm of absolute histogram difference in `plane` of the regions, towards whichever side has room"""
        for r in self._regions(which):
            self.m[r, plane] += dm if self.m[r, plane] + dm <= self.n else -dm
            assert 0 <= self.m[r, plane] <= self.n, (r, plane, dm)

    def cut(self, which, planes=(0, 1, 2), light=0):
        """another bin pair: 2 * N of difference in every plane named; the intensity byte moves by `light`"""
        for r in self._regions(which):
            for p in planes:
                self.pair[r, p] = (self.pair[r, p] + 1) % 16
            self.light([r], light)

    def light(self, which, d):
        for r in self._regions(which):
            self.avg[r] += d if self.avg[r] + d <= 255 else -d
            assert 0 <= self.avg[r] <= 255

    def emit(self, flash=None):
        """the next picture; flash = (regions, dm, light): a step and a light that this picture alone has"""
        m, avg = self.m.copy(), self.avg.copy()
        if flash:
            keep = self.m.copy(), self.avg.copy()
            self.step(flash[0], 0, flash[1]), self.light(flash[0], flash[2])
            m, avg = self.m.copy(), self.avg.copy()
            self.m, self.avg = keep
        hist = self.floor.copy()
        for r in range(self.regions):
            for p in range(3):
                hist[r, p, 10 + 7 * self.pair[r, p]] += self.n - m[r, p]
                hist[r, p, 130 + 7 * self.pair[r, p]] += m[r, p]
        row = np.zeros(64, np.uint8)
        row[:self.regions] = avg
        detect = np.zeros(1, PIC_DETECT_DTYPE)
        detect["pic_avg_variance"] = self.var
        self.pictures.append(dict(luma=np.ascontiguousarray(hist[:, 0]).astype(np.uint32), chroma=np.ascontiguousarray(hist[:, 1:]).astype(np.uint32),
                                  avg=row, detect=detect))

    def run(self, jobs, events):
        """events: picture index -> a function of the script, called before that picture is emitted"""
        for p in range(jobs + 2):
            flash = events[p](self) if p in events else None
            self.emit(flash)
        return self.pictures


def _cut(which=ALL, light=20, planes=(0, 1, 2)):
    return lambda s: s.cut(which, planes, light)


def _step(which, plane, dm, light=0):
    def f(s):
        s.step(which, plane, dm), s.light(which, light)
    return f


def _flash(which, dm, light):
    return lambda s: (which, dm, light)


def _var(value, then=None):
    def f(s):
        s.var = value
        return then(s) if then else None
    return f


def long_events(jobs, seed):
    """a seeded mix of everything above, one event in about every third picture"""
    rng = np.random.default_rng(seed)
    events = {}
    for p in range(1, jobs + 2):
        u = rng.random()
        some = sorted(rng.choice(16, int(rng.integers(1, 17)), replace=False).tolist())
        if u < 0.10:
            events[p] = _cut(some, int(rng.integers(5, 40)))
        elif u < 0.15:
            events[p] = _flash(some, int(rng.integers(1600, 2500)), int(rng.integers(6, 30)))
        elif u < 0.20:
            events[p] = _cut(some, int(rng.integers(0, 3)))                        # a fade
        elif u < 0.27:
            events[p] = _step(some, 0, int(rng.integers(1501, 3001)), int(rng.integers(0, 9)))   # gradual from a settled average
        elif u < 0.31:
            events[p] = _step(some, int(rng.integers(1, 3)), int(rng.integers(760, 2000)), int(rng.integers(0, 12)))
        elif u < 0.35:
            events[p] = _var(int(rng.choice([600, 1100, 2100, 2600])), _step(some, 0, int(rng.integers(2400, 4000)), 7))
        elif u < 0.60:
            events[p] = _step(some, int(rng.integers(0, 3)), int(rng.integers(1, 300)))          # below every threshold
    return events


# name -> (w, h, rw, rh, scd_mode, jobs, seed, events).  The inequality each event plants is spelled out in tests/golden/make_scd_golden.py:assert_not_vacuous
# and asserted there on the reference's results.  Thresholds: T * ((w // rw) * (h // rh) >> 12) where both remainders are 0.
CASES = {
    # 128x80 regions: th 6000, chroma 1500, vote 8
    "cut_512x320": (512, 320, 4, 4, 1, 12, 101, {6: _cut()}),
    # a flash in picture 3 alone, a fade in picture 7, a cut in 7 regions at picture 10 and in 8 at picture 13
    "flash_fade_512x320": (512, 320, 4, 4, 1, 16, 102, {3: _flash(ALL, 4000, 20), 7: _cut(ALL, 2), 10: _cut(list(range(7)), 25), 13: _cut(list(range(4, 12)), 25)}),
    # 160x96 regions: th 9000, chroma 2250
    "chroma_only_640x384": (640, 384, 4, 4, 1, 10, 103, {3: _step(ALL, 1, 2000, 12), 7: _step(ALL, 2, 2000, 12)}),
    # 480x272 regions: 31 units, th 93000 / 139500.  Pictures 3..7: sums of 90000, 112000, 135000, 160000, 183000 - each within th of the average, which
    # climbs to 113665; picture 8 is still: its error exceeds th but its sum (0) does not reach it.  Picture 10 a cut (reset); picture 13 a sum of 120000 with
    # the variance stepping from 600 to 2100: gradual under 139500, where 93000 would have made it a scene change
    "gradual_noise_1920x1088": (1920, 1088, 4, 4, 1, 16, 104, {3: _step(ALL, 0, 45000), 4: _step(ALL, 0, 56000), 5: _step(ALL, 0, 67500), 6: _step(ALL, 0, 80000),
                                                              7: _step(ALL, 0, 91500), 10: _cut(), 13: _var(2100, _step(ALL, 0, 60000, 20))}),
    # 173x109 + remainders of 1: every accumulated size still has 4 units (th 12000); mode 2: vote 7.  A cut in 6 regions, then in 7
    "ragged_520x328_r3": (520, 328, 3, 3, 2, 8, 105, {3: _cut(list(range(6)), 25), 6: _cut(list(range(2, 9)), 25)}),
    # 178x114 + remainders of 2: the heights run 114, 116, 112, 120 and the last column's widths 180, 176, 184 - regions 2, 3, 4 and 8 have 5 units (th 15000),
    # the others 4 (th 12000): a sum of 13500 is abrupt in five regions and gradual in four
    "ragged_536x344_r3": (536, 344, 3, 3, 2, 8, 106, {3: _step(ALL, 0, 6750, 20), 6: _cut()}),
    "one_region_64x64": (64, 64, 1, 1, 1, 4, 107, {3: _cut()}),
    # 64x64 regions: one unit, th 3000, chroma 750
    "tiny_256x128": (256, 128, 4, 2, 1, 6, 108, {3: _step(ALL, 1, 500, 9)}),
    # 32x32 regions: (w * h) >> 12 is 0 and both thresholds are 0 - one sample moved is an abrupt change; vote 4
    "zero_th_128x64": (128, 64, 4, 2, 1, 6, 109, {3: _step([0, 3, 5, 6], 0, 1, 9)}),
    # 18x19 regions with a height remainder of 2: the heights run 19, 21, 15, 33 and 19 - 40 = -21 in the last region, a large unsigned number whose product and
    # threshold wrap; every other region has 0 units
    "wrap_72x78": (72, 78, 4, 4, 1, 6, 110, {3: _step(ALL, 0, 3, 9)}),
    "long_256": (512, 320, 4, 4, 1, 256, 111, None),
}
ISSUE_CASES = ("cut_512x320", "flash_fade_512x320", "chroma_only_640x384", "gradual_noise_1920x1088", "ragged_520x328_r3", "one_region_64x64", "tiny_256x128",
               "long_256")


def case_pictures(name):
    w, h, rw, rh, mode, jobs, seed, events = CASES[name]
    return Script(w, h, rw, rh, seed).run(jobs, long_events(jobs, seed) if events is None else events)


def window(pictures, i):
    """job i of a case: (past, current, future)"""
    return pictures[i], pictures[i + 1], pictures[i + 2]


def case_windows(name):
    """the (past, current, future) pictures of every job of a case"""
    pictures = case_pictures(name)
    return [window(pictures, i) for i in range(CASES[name][5])]


def load_case(name):
    """the fixture of a case (tests/golden/scd_<name>.npz): what the reference's own function left after every job"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scd_%s.npz" % name))
    assert str(g["case"][0]) == name
    return {k: g[k] for k in g.files}


def write_case(f, w, h, rw, rh, mode, windows, state=None):
    """one case of the file tools/scd_logic_check.c reads: a header of seven int32 (w, h, rw, rh, scd_mode, jobs, whether a state follows), the state, then per job
    the histograms of the past and the current picture (luma, then chroma), the three luma average rows CUT to the regions, and the two variances"""
    f.write(np.array([w, h, rw, rh, mode, len(windows), state is not None], np.int32).tobytes())
    if state is not None:
        assert state.dtype == STATE_DTYPE and state.size == 1
        f.write(state.tobytes())
    n = rw * rh
    for past, cur, future in windows:
        f.write(past["luma"].tobytes() + cur["luma"].tobytes() + past["chroma"].tobytes() + cur["chroma"].tobytes())
        f.write(past["avg"][:n].tobytes() + cur["avg"][:n].tobytes() + future["avg"][:n].tobytes())
        f.write(np.array([past["detect"]["pic_avg_variance"][0], cur["detect"]["pic_avg_variance"][0]], "<u2").tobytes())


def split_outputs(raw, jobs):
    """the check program's output file -> the three arrays"""
    cuts = np.cumsum([jobs * PIC_DTYPE.itemsize, jobs * 192, jobs * STATE_DTYPE.itemsize])
    assert len(raw) == cuts[-1], (len(raw), cuts)
    pic, ahd, state = np.split(raw, cuts[:-1])
    return dict(picture=pic.view(PIC_DTYPE), ahd=ahd.view(AHD_DTYPE).reshape(jobs, 16, 3), state=state.view(STATE_DTYPE))


def same(got, want, tag):
    """the three arrays byte for byte, pads included"""
    for k in ("picture", "ahd", "state"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))
            raise AssertionError((tag, k, "first differing job", int(bad[0]) // (a.nbytes // len(a))))
