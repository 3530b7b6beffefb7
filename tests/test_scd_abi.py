"""CPU-only: the C-ABI of the batched scene-transition detection (include/svt_hevc_amd.h "Batched scene-transition detection") - the entries are exported, the
header, the ctypes views (tests/scdlib.py) and the numpy layouts (tests/scd_records.py) agree on sizes and offsets, the checks that need no device answer
without one, and svt_amd_scene_detect_bytes is the documented arithmetic."""
import ctypes as C

import pytest

import scd_records as R
import scdlib as M
from abi_util import compiles, exported, open_library, view_matches_dtype
from pa_batch_util import refused, refused_as

VIEWS = (("SvtAmdScdJob", M.ScdJob), ("SvtAmdScdPic", M.ScdPic), ("SvtAmdScdState", M.ScdState), ("SvtAmdScdArrays", M.ScdArrays))


@pytest.fixture(scope="module")
def lib():
    return open_library(M.declare)


def test_entries_are_exported():
    assert {"svt_amd_scene_detect_batch_launch", "svt_amd_scene_detect_bytes", "svt_amd_debug_scene_detect_stages"} <= exported()


def test_structure_sizes_in_c99(tmp_path):
    """sizeof of the structures as a C99 compiler sees the header (_Static_assert is gcc's extension there), against the ctypes views and the numpy layouts"""
    assert (R.PIC_DTYPE.itemsize, R.STATE_DTYPE.itemsize, R.PIC_DETECT_DTYPE.itemsize) == (24, 196, 8)
    assert C.sizeof(M.ScdJob) == 72 and C.sizeof(M.ScdArrays) == 24
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS]
    checks += ["SVT_AMD_SCD_PICTURE == 0 && SVT_AMD_SCD_AHD == 1 && SVT_AMD_SCD_STATE == 2", "SVT_AMD_SCD_MAX_LCUS == %d" % M.MAX_LCUS,
               "SVT_AMD_SCD_MAX_REGIONS == %d" % M.MAX_REGIONS, "sizeof(SvtAmdPaPicDetect) == %d" % R.PIC_DETECT_DTYPE.itemsize,
               "SVT_AMD_SCD_CLASS_NONE == %d && SVT_AMD_SCD_CLASS_GRADUAL == %d && SVT_AMD_SCD_CLASS_FLASH == %d && SVT_AMD_SCD_CLASS_FADE == %d && "
               "SVT_AMD_SCD_CLASS_SCENE == %d" % (R.NONE, R.GRADUAL, R.FLASH, R.FADE, R.SCENE)]
    compiles(tmp_path, "c99", checks)


def test_header_offsets_field_by_field(tmp_path):
    """every field of the header's structures lies where the ctypes view has it"""
    compiles(tmp_path, "c11", ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_])


@pytest.mark.parametrize("view,dtype", [(M.ScdPic, R.PIC_DTYPE), (M.ScdState, R.STATE_DTYPE)])
def test_ctypes_views_have_the_dtypes_offsets(view, dtype):
    view_matches_dtype(view, dtype)


def launch(lib, ctx, jobs, n, table, w=64, h=64, rw=4, rh=4, mode=1):
    return lib.svt_amd_scene_detect_batch_launch(ctx, jobs, n, w, h, rw, rh, mode, None, table)


def test_bad_headers_are_refused_without_a_device(lib):
    jobs, table = (M.ScdJob * 1)(), M.ScdArrays()
    refused(lib, launch(lib, None, jobs, 1, C.byref(table)), M.ENTRY)
    fake = C.create_string_buffer(4096)          # never read: everything below is checked in front of the context
    for n in (0, -1, 257, 1 << 20):
        refused(lib, launch(lib, fake, jobs, n, C.byref(table)), M.ENTRY, n)
    refused(lib, launch(lib, fake, None, 1, C.byref(table)), M.ENTRY)
    refused(lib, launch(lib, fake, jobs, 1, None), M.ENTRY)
    for rw, rh in ((0, 4), (4, 0), (5, 4), (4, 5), (-1, 1)):
        refused_as(lib, launch(lib, fake, jobs, 1, C.byref(table), rw=rw, rh=rh), M.ENTRY + ": %d x %d regions (1..4 each)" % (rw, rh))
    for mode in (0, 3):
        refused_as(lib, launch(lib, fake, jobs, 1, C.byref(table), mode=mode), M.ENTRY + ": scd_mode %d (1..2)" % mode)
    refused_as(lib, launch(lib, fake, jobs, 1, C.byref(table), w=0), M.ENTRY + ": a picture of 0x64 (at least 8x8)")
    refused_as(lib, launch(lib, fake, jobs, 1, C.byref(table), h=0), M.ENTRY + ": a picture of 64x0 (at least 8x8)")
    # the bound of the kernels: the words the batched entries share
    refused_as(lib, launch(lib, fake, jobs, 1, C.byref(table), w=16384, h=16384), M.ENTRY + ": job 0: a picture of 16384x16384 (at most 16384 LCUs)")


@pytest.mark.parametrize("rw,rh", [(1, 1), (3, 3), (4, 2), (4, 4)])
def test_bytes_per_job_are_the_documented_sizes(lib, rw, rh):
    assert lib.svt_amd_scene_detect_bytes(M.SCD_PICTURE, rw, rh) == R.PIC_DTYPE.itemsize
    assert lib.svt_amd_scene_detect_bytes(M.SCD_AHD, rw, rh) == 16 * 3 * 4
    assert lib.svt_amd_scene_detect_bytes(M.SCD_STATE, rw, rh) == R.STATE_DTYPE.itemsize
    for which in (-1, 3, 99):
        assert lib.svt_amd_scene_detect_bytes(which, rw, rh) == 0
    for bad in ((0, rh), (rw, 0), (5, rh), (rw, 5)):
        assert lib.svt_amd_scene_detect_bytes(M.SCD_PICTURE, *bad) == 0
