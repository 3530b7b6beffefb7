"""Helpers of the batched side-statistics tests (svt_amd_side_stats_batch_launch, svt-hevc_amd/csrc/side_kernels.hip): ctypes mirrors of the two
structures, the per-picture array sizes in numpy terms, a batch runner that hands back every array as numpy, and the three blocking single-picture
entries for the same slots."""
import ctypes as C

import numpy as np

import svtlib as S
from pa_batch_util import BAD_PARAM, SENTINEL, DeviceBuffer  # noqa: F401 (the two constants are used through this module)

vp = C.c_void_p
BLOCK_STATS, AC_ENERGY, ZZ_SAD, HISTOGRAM, REGION_AVG, SUM_LUMA = range(6)
KINDS = ("block_stats", "ac_energy", "zz", "histogram", "region_average", "sum_luma")
ZZ_DTYPE = np.dtype([("sad", "<u4"), ("zz_cost", "u1"), ("non_moving_index", "u1"), ("pad", "u1", 2)])
NOT_COMPUTED = 100000000           # the AC energy of an incomplete LCU


class SideJob(C.Structure):
    _fields_ = [("cur_slot", C.c_int32), ("prev_slot", C.c_int32), ("want_block_stats", C.c_uint8), ("want_ac_energy", C.c_uint8),
                ("want_histogram", C.c_uint8), ("pad", C.c_uint8)]


class SideArrays(C.Structure):
    _fields_ = [(k, vp) for k in KINDS]


def declare(lib):
    lib.svt_amd_last_error.restype = C.c_char_p
    lib.svt_amd_side_stats_batch_launch.restype = C.c_int
    lib.svt_amd_side_stats_batch_launch.argtypes = [vp, C.POINTER(SideJob), C.c_int, C.c_int, C.c_int, C.POINTER(SideArrays)]
    lib.svt_amd_side_stats_bytes.restype = C.c_size_t
    lib.svt_amd_side_stats_bytes.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_int]
    lib.svt_amd_picture_stats.restype, lib.svt_amd_picture_stats.argtypes = C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.svt_amd_picture_ac_energy.restype, lib.svt_amd_picture_ac_energy.argtypes = C.c_int, [vp, C.c_int, vp]
    lib.svt_amd_zz_sad_picture.restype, lib.svt_amd_zz_sad_picture.argtypes = C.c_int, [vp, C.c_int, C.c_int, vp]
    return lib


def numpy_sizes(w, h, rw, rh):
    """bytes of ONE picture in each array, from the numpy side"""
    n = S.lcu_count(w, h)
    return [n * S.PA_LCU_STATS_DTYPE.itemsize, n * 40, n * 8, rw * rh * 1024, 64, 8]


def make_jobs(spec):
    """spec: (cur_slot, prev_slot, want_block_stats, want_ac_energy, want_histogram) per picture"""
    jobs = (SideJob * len(spec))()
    for j, (cur, prev, bs, ac, hist) in zip(jobs, spec):
        j.cur_slot, j.prev_slot, j.want_block_stats, j.want_ac_energy, j.want_histogram = cur, prev, int(bs), int(ac), int(hist)
    return jobs


def all_jobs(slots, first_prev=-1):
    """every result of every slot; the previous picture of slot i is slot i - 1"""
    return make_jobs([(s, slots[i - 1] if i else first_prev, 1, 1, 1) for i, s in enumerate(slots)])


class DeviceArrays:
    """the six device arrays of an n-picture batch, filled with SENTINEL"""

    def __init__(self, lib, ctx, n, w, h, rw=4, rh=4, absent=()):
        self.n, self.rw, self.rh = n, rw, rh
        self.sizes = numpy_sizes(w, h, rw, rh)
        self.buf = [None if KINDS[k] in absent else DeviceBuffer(lib, ctx, n * b) for k, b in enumerate(self.sizes)]
        self.ptr = [b.ptr if b else vp() for b in self.buf]

    def fill(self):
        for b in filter(None, self.buf):
            b.fill()

    def table(self):
        return SideArrays(*[p.value for p in self.ptr])

    def raw(self, k):
        return self.buf[k].get().reshape(self.n, -1)

    def download(self):
        """blocking copies (they wait for the context's stream): the arrays as numpy, picture first"""
        return views([self.raw(k) if self.buf[k] else None for k in range(6)], self.n, self.rw, self.rh)

    def free(self):
        for b in filter(None, self.buf):
            b.free()
        self.buf, self.ptr = [None] * 6, [vp() for _ in KINDS]


def views(raw, n, rw, rh):
    """raw: the six byte arrays [n][bytes per picture] (or None) -> dict of typed arrays"""
    out = {}
    if raw[BLOCK_STATS] is not None:
        out["block_stats"] = raw[BLOCK_STATS].view(S.PA_LCU_STATS_DTYPE).reshape(n, -1)
    if raw[AC_ENERGY] is not None:
        out["ac_energy"] = raw[AC_ENERGY].view(np.uint64).reshape(n, -1, 5)
    if raw[ZZ_SAD] is not None:
        out["zz"] = raw[ZZ_SAD].view(ZZ_DTYPE).reshape(n, -1)
    if raw[HISTOGRAM] is not None:
        out["histogram"] = raw[HISTOGRAM].view(np.uint32).reshape(n, rw, rh, 256)
    if raw[REGION_AVG] is not None:
        out["region_average"] = raw[REGION_AVG].reshape(n, 64)
    if raw[SUM_LUMA] is not None:
        out["sum_luma"] = raw[SUM_LUMA].view(np.uint64).reshape(n)
    return out


def launch(lib, ctx, jobs, arrays, rw=4, rh=4):
    t = arrays.table() if isinstance(arrays, DeviceArrays) else arrays
    return lib.svt_amd_side_stats_batch_launch(ctx, jobs, len(jobs), rw, rh, C.byref(t))


def run_batch(lib, ctx, jobs, w, h, rw=4, rh=4):
    """one batch into fresh arrays; returns the typed arrays"""
    arrays = DeviceArrays(lib, ctx, len(jobs), w, h, rw, rh)
    try:
        assert launch(lib, ctx, jobs, arrays, rw, rh) == 0, lib.svt_amd_last_error()
        return arrays.download()
    finally:
        arrays.free()


def blocking_picture(lib, ctx, slot, prev_slot, w, h, rw=4, rh=4):
    """the three blocking single-picture entries for a slot: (block_stats, histogram, region_average[rw * rh], sum_luma, ac_energy, zz or None)"""
    n = S.lcu_count(w, h)
    stats = np.zeros(n, S.PA_LCU_STATS_DTYPE)
    hist, ravg, total = np.zeros((rw, rh, 256), np.uint32), np.zeros(rw * rh, np.uint8), C.c_uint64(0)
    assert lib.svt_amd_picture_stats(ctx, slot, stats.ctypes.data, rw, rh, hist.ctypes.data, ravg.ctypes.data, C.byref(total)) == 0, lib.svt_amd_last_error()
    energy = np.zeros((n, 5), np.uint64)
    assert lib.svt_amd_picture_ac_energy(ctx, slot, energy.ctypes.data) == 0, lib.svt_amd_last_error()
    zz = None
    if prev_slot >= 0:
        zz = np.zeros(n, ZZ_DTYPE)
        assert lib.svt_amd_zz_sad_picture(ctx, slot, prev_slot, zz.ctypes.data) == 0, lib.svt_amd_last_error()
    return stats, hist, ravg, int(total.value), energy, zz


def assert_equals_blocking(lib, ctx, got, i, slot, prev_slot, w, h, rw=4, rh=4, what=""):
    """picture i of a batch against the blocking entries for the same slots, byte for byte (padding bytes included)"""
    stats, hist, ravg, total, energy, zz = blocking_picture(lib, ctx, slot, prev_slot, w, h, rw, rh)
    assert got["block_stats"][i].tobytes() == stats.tobytes(), (what, i, "block_stats")
    assert got["ac_energy"][i].tobytes() == energy.tobytes(), (what, i, "ac_energy")
    assert got["histogram"][i].tobytes() == hist.tobytes(), (what, i, "histogram")
    assert got["region_average"][i].tobytes() == ravg.tobytes() + bytes(64 - rw * rh), (what, i, "region_average")
    assert int(got["sum_luma"][i]) == total, (what, i, "sum_luma")
    if zz is not None:
        assert got["zz"][i].tobytes() == zz.tobytes(), (what, i, "zz")
