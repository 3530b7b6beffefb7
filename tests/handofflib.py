"""ctypes views, numpy layouts and prototypes of the stream-ordered entropy hand-off (include/svt_hevc_amd.h "Entropy hand-off pre-scan":
svt_amd_entropy_handoff_bytes, svt_amd_entropy_handoff_launch, svt_amd_encdec_picture_entropy_handoff) and of the blocking svt_amd_coeff_scan_picture;
tests/test_handoff_abi.py holds them against the header.  Outputs: one launch's output arrays in device memory, each with sentinel bytes behind it.  scan_picture:
the blocking entry into host arrays, sentinel behind the capacities."""
import ctypes as C

import numpy as np

import svtlib as S
from pa_batch_util import SENTINEL, DeviceBuffer, is_sentinel, round_up

ENTRY = "svt_amd_entropy_handoff_launch"
PICTURE_ENTRY = "svt_amd_encdec_picture_entropy_handoff"
BLOCKING_ENTRY = "svt_amd_coeff_scan_picture"
ERR_RESOURCES = -2                 # SVT_AMD_ERR_RESOURCES
SLACK = 64                         # sentinel elements the host lists of scan_picture keep behind their capacity
HEAD, LCUS, GROUPS, LEVELS, WORK_HEADS, RESULT_HEADS = range(6)   # SVT_AMD_ENTROPY_HANDOFF_*
MAX_LCUS = 16384                   # SVT_AMD_MDCTL_MAX_LCUS
MAX_GROUPS, MAX_LEVELS = 384, 6144  # an LCU's worst case
WORK_HEAD_BYTES = 1584             # head + unit list of SvtAmdLcuWork[16]
RESULT_HEAD_BYTES = 768            # SvtAmdLcuCuResult[64]
RESULT_MIN_BYTES = 768 + 2 * (4096 + 2 * 1024)   # offsetof(SvtAmdLcuResult, rec_y)
NONE = 0xFFFFFFFF
GUARD = 256                        # sentinel bytes kept behind every output array
u16, u32, vp = C.c_uint16, C.c_uint32, C.c_void_p


class Head(C.Structure):
    _fields_ = [("groups", u32), ("levels", u32), ("overflow", u32), ("bad_lcus", u32), ("first_bad_lcu", u32), ("bad_units", u32), ("first_bad_unit_lcu", u32),
                ("pad", u32)]


class Job(C.Structure):
    _fields_ = [("d_works", vp), ("work_stride", C.c_size_t), ("d_results", vp), ("result_stride", C.c_size_t), ("n_lcus", u32), ("group_capacity", u32),
                ("level_capacity", u32), ("pad", u32)]


class Out(C.Structure):
    _fields_ = [("head", vp), ("lcus", vp), ("groups", vp), ("levels", vp), ("work_heads", vp), ("result_heads", vp)]


HEAD_DTYPE = np.dtype([(f, "<u4") for f, _ in Head._fields_])
LCU_BYTES = S.COEFF_SCAN_LCU_DTYPE.itemsize          # 1552
assert C.sizeof(Head) == 32 and C.sizeof(Job) == 48 and C.sizeof(Out) == 48 and HEAD_DTYPE.itemsize == 32
assert S.LCU_WORK_DTYPE.fields["src_y"][1] == WORK_HEAD_BYTES and S.LCU_RESULT_DTYPE.fields["coeff_y"][1] == RESULT_HEAD_BYTES
assert S.LCU_RESULT_DTYPE.fields["rec_y"][1] == RESULT_MIN_BYTES == S.LCU_RESULT16_DTYPE.fields["rec_y"][1]


def declare(lib):
    lib.svt_amd_entropy_handoff_bytes.restype, lib.svt_amd_entropy_handoff_bytes.argtypes = C.c_size_t, [u16, u16, C.c_int]
    lib.svt_amd_entropy_handoff_launch.restype, lib.svt_amd_entropy_handoff_launch.argtypes = C.c_int, [vp, vp, vp]
    lib.svt_amd_encdec_picture_entropy_handoff.restype, lib.svt_amd_encdec_picture_entropy_handoff.argtypes = C.c_int, [vp, vp, u32, u32, vp]
    lib.svt_amd_coeff_scan_picture.restype = C.c_int
    lib.svt_amd_coeff_scan_picture.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp, vp, u32, vp, u32, C.POINTER(u32 * 2)]
    lib.svt_amd_synchronize.restype, lib.svt_amd_synchronize.argtypes = C.c_int, [vp]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib


def job(d_works, work_stride, d_results, result_stride, n, gcap, lcap):
    j = Job()
    j.d_works, j.work_stride, j.d_results, j.result_stride, j.n_lcus, j.group_capacity, j.level_capacity = d_works, work_stride, d_results, result_stride, n, gcap, lcap
    return j


class Outputs:
    """the six output arrays of one launch in ONE device allocation filled with the sentinel, GUARD sentinel bytes behind each; capacities in elements"""

    def __init__(self, lib, ctx, n, gcap, lcap, heads=True):
        self.n, self.gcap, self.lcap, self.heads = n, gcap, lcap, heads
        sizes = [("head", 32), ("lcus", n * LCU_BYTES), ("groups", 8 * gcap), ("levels", 2 * lcap)]
        if heads:
            sizes += [("work_heads", n * WORK_HEAD_BYTES), ("result_heads", n * RESULT_HEAD_BYTES)]
        self.at, self.size, off = {}, dict(sizes), 0
        for name, b in sizes:
            self.at[name] = off
            off += round_up(b + GUARD)
        self.dev = DeviceBuffer(lib, ctx, off)
        self.out = Out()
        for name, _ in sizes:
            setattr(self.out, name, self.dev.at(self.at[name]))

    def get(self):
        """downloaded (waits for the context's stream): dict of arrays; the bytes behind every array must be the sentinel"""
        raw = self.dev.get()
        part = {}
        for name, b in self.size.items():
            at = self.at[name]
            end = at + round_up(b + GUARD)
            assert is_sentinel(raw[at + b:end]), "bytes behind " + name
            part[name] = raw[at:at + b]
        got = {"head": part["head"].view(HEAD_DTYPE)[0], "lcus": part["lcus"].view(S.COEFF_SCAN_LCU_DTYPE), "groups": part["groups"].view(S.COEFF_SCAN_GROUP_DTYPE),
               "levels": part["levels"].view(np.uint16), "raw": part}
        if self.heads:
            got["work_heads"] = part["work_heads"].reshape(self.n, WORK_HEAD_BYTES)
            got["result_heads"] = part["result_heads"].reshape(self.n, RESULT_HEAD_BYTES)
        return got

    def untouched(self):
        return is_sentinel(self.dev.get())

    def free(self):
        self.dev.free()


def scan_picture(lib, ctx, works, work_stride, results, result_stride, device_arrays, n, gcap, lcap):
    """svt_amd_coeff_scan_picture on record arrays given by address, into host arrays filled with the sentinel, the lists SLACK elements longer than the
    capacities the call is told: (return code, {lcus, groups, levels: the whole arrays; totals})"""
    lcus = np.full(n * LCU_BYTES, SENTINEL, np.uint8).view(S.COEFF_SCAN_LCU_DTYPE)
    groups = np.full(8 * (gcap + SLACK), SENTINEL, np.uint8).view(S.COEFF_SCAN_GROUP_DTYPE)
    levels = np.full(2 * (lcap + SLACK), SENTINEL, np.uint8).view(np.uint16)
    totals = (u32 * 2)(NONE, NONE)
    rc = lib.svt_amd_coeff_scan_picture(ctx, vp(works), work_stride, vp(results), result_stride, device_arrays, n, lcus.ctypes.data, groups.ctypes.data, gcap,
                                        levels.ctypes.data, lcap, C.byref(totals))
    return rc, {"lcus": lcus, "groups": groups, "levels": levels, "totals": (int(totals[0]), int(totals[1]))}
