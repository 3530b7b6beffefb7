"""CPU-only: the C-ABI of the batched initial rate control (include/svt_hevc_amd.h "Batched initial rate control") - the entries are exported, the header, the
ctypes views (tests/irclib.py) and the numpy layouts (tests/irc_records.py) agree on sizes and offsets, the checks that need no device answer without one, and
svt_amd_initial_rc_bytes is the documented arithmetic."""
import ctypes as C

import pytest

import irc_records as R
import irclib as M
import svtlib as S
from abi_util import compiles, exported, open_library, view_matches_dtype
from pa_batch_util import refused, refused_as

VIEWS = (("SvtAmdIrcJob", M.IrcJob), ("SvtAmdIrcChecks", M.IrcChecks), ("SvtAmdIrcMotion", M.IrcMotion), ("SvtAmdIrcLcu", M.IrcLcu), ("SvtAmdIrcPic", M.IrcPic),
         ("SvtAmdIrcArrays", M.IrcArrays))


@pytest.fixture(scope="module")
def lib():
    return open_library(M.declare)


def test_entries_are_exported():
    assert {"svt_amd_initial_rc_batch_launch", "svt_amd_initial_rc_bytes"} <= exported()


def test_structure_sizes_in_c99(tmp_path):
    """sizeof of the structures as a C99 compiler sees the header (_Static_assert is gcc's extension there), against the ctypes views and the numpy layouts"""
    assert (R.CHECKS_DTYPE.itemsize, R.MOTION_DTYPE.itemsize, R.IRC_LCU_DTYPE.itemsize, R.IRC_PIC_DTYPE.itemsize) == (4, 24, 48, 16)
    assert C.sizeof(M.IrcJob) == 288
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS]
    checks += ["SVT_AMD_IRC_CHECKS == 0 && SVT_AMD_IRC_MOTION == 1 && SVT_AMD_IRC_LCU == 2 && SVT_AMD_IRC_STATIONARY == 3 && SVT_AMD_IRC_PM_STATIONARY == 4",
               "SVT_AMD_IRC_PICTURE == 5", "SVT_AMD_IRC_MAX_LCUS == %d" % M.MAX_LCUS]
    compiles(tmp_path, "c99", checks)


def test_header_offsets_field_by_field(tmp_path):
    """every field of the header's structures lies where the ctypes view has it"""
    compiles(tmp_path, "c11", ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_])


@pytest.mark.parametrize("view,dtype", [(M.IrcChecks, R.CHECKS_DTYPE), (M.IrcMotion, R.MOTION_DTYPE), (M.IrcLcu, R.IRC_LCU_DTYPE), (M.IrcPic, R.IRC_PIC_DTYPE)])
def test_ctypes_views_have_the_dtypes_offsets(view, dtype):
    view_matches_dtype(view, dtype)


def test_job_layout():
    assert M.IrcJob.edge_checks.offset == 16 and M.IrcJob.edge_detect.offset == 48 and M.IrcJob.hom_stats.offset == 80 and M.IrcJob.pan_motion.offset == 208
    assert M.IrcJob.cur_slot.offset == 272 and M.IrcJob.edge_count.offset == 276 and M.IrcJob.frames_to_check.offset == 284 and M.IrcJob.pad.offset == 285


def test_bad_headers_are_refused_without_a_device(lib):
    jobs, table = (M.IrcJob * 1)(), M.IrcArrays()
    refused(lib, lib.svt_amd_initial_rc_batch_launch(None, jobs, 1, 64, 64, C.byref(table)), M.ENTRY)
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_initial_rc_batch_launch(fake, jobs, n, 64, 64, C.byref(table)), M.ENTRY, n)
    refused(lib, lib.svt_amd_initial_rc_batch_launch(fake, None, 1, 64, 64, C.byref(table)), M.ENTRY)
    refused(lib, lib.svt_amd_initial_rc_batch_launch(fake, jobs, 1, 64, 64, None), M.ENTRY)
    # ... nor for the picture's size: the bound of the kernels is tested before the context's own
    refused_as(lib, lib.svt_amd_initial_rc_batch_launch(fake, jobs, 1, 0, 64, C.byref(table)), M.ENTRY + ": job 0: a picture of 0x64 (at most 16384 LCUs)")
    refused_as(lib, lib.svt_amd_initial_rc_batch_launch(fake, jobs, 1, 16384, 16384, C.byref(table)), M.ENTRY + ": job 0: a picture of 16384x16384 (at most 16384 LCUs)")


@pytest.mark.parametrize("w,h", [(64, 64), (416, 240), (2112, 1152), (3840, 2160)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h):
    n = S.lcu_count(w, h)
    assert lib.svt_amd_initial_rc_bytes(w, h, M.IRC_CHECKS) == n * R.CHECKS_DTYPE.itemsize
    assert lib.svt_amd_initial_rc_bytes(w, h, M.IRC_MOTION) == R.MOTION_DTYPE.itemsize
    assert lib.svt_amd_initial_rc_bytes(w, h, M.IRC_LCU) == n * R.IRC_LCU_DTYPE.itemsize
    assert lib.svt_amd_initial_rc_bytes(w, h, M.IRC_STATIONARY) == lib.svt_amd_initial_rc_bytes(w, h, M.IRC_PM_STATIONARY) == (n + 63) // 64 * 64
    assert lib.svt_amd_initial_rc_bytes(w, h, M.IRC_PICTURE) == R.IRC_PIC_DTYPE.itemsize
    for which in (-1, 6, 99):
        assert lib.svt_amd_initial_rc_bytes(w, h, which) == 0
