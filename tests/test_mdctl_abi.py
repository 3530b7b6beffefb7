"""CPU-only: the C-ABI of the batched mode-decision LCU controls (include/svt_hevc_amd.h "Batched mode-decision LCU controls") - the entries are exported, the
header, the ctypes views (tests/mdctllib.py) and the numpy layouts (svtlib.MD_LCU_DTYPE, mdctl_records.CHECK_DTYPE) agree on sizes and offsets, the head of
SvtAmdMdcLcu is the head of SvtAmdMdLcu, the checks that need no device answer without one, and svt_amd_md_controls_bytes is the documented arithmetic."""
import ctypes as C

import pytest

import mdclib as MM
import mdc_records as MR
import mdctl_records as R
import mdctllib as M
import svtlib as S
from abi_util import compiles, exported, open_library, view_matches_dtype
from pa_batch_util import BAD_PARAM, refused, refused_as

VIEWS = (("SvtAmdMdCtlJob", M.MdCtlJob), ("SvtAmdMdLcu", M.MdLcu), ("SvtAmdMdCtlCheck", M.MdCtlCheck), ("SvtAmdMdcLcu", MM.MdcLcu))


@pytest.fixture(scope="module")
def lib():
    return open_library(M.declare)


def test_entries_are_exported():
    assert {"svt_amd_md_controls_batch_launch", "svt_amd_md_controls_bytes", "svt_amd_md_picture_set_controls", "svt_amd_debug_md_controls_check"} <= exported()


def test_structure_sizes_in_c99(tmp_path):
    """sizeof of the structures as a C99 compiler sees the header (_Static_assert is gcc's extension there), against the ctypes views and the numpy layouts"""
    assert (C.sizeof(M.MdCtlJob), C.sizeof(M.MdLcu), C.sizeof(M.MdCtlCheck)) == (88, 191, 88)
    assert (S.MD_LCU_DTYPE.itemsize, R.CHECK_DTYPE.itemsize) == (191, 88)
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS]
    checks += ["SVT_AMD_MDCTL_LCU == 0", "SVT_AMD_MDCTL_MAX_LCUS == %d" % M.MAX_LCUS, "SVT_AMD_MD_LEAVES == 85"]
    compiles(tmp_path, "c99", checks)


def test_header_offsets_field_by_field(tmp_path):
    """every field of the header's structures lies where the ctypes view has it"""
    compiles(tmp_path, "c11", ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_])


@pytest.mark.parametrize("view,dtype", [(M.MdLcu, S.MD_LCU_DTYPE), (M.MdCtlCheck, R.CHECK_DTYPE), (MM.MdcLcu, MR.MDC_LCU_DTYPE)])
def test_ctypes_views_have_the_dtypes_offsets(view, dtype):
    view_matches_dtype(view, dtype)


def test_the_head_of_the_configuration_record_is_the_head_of_the_control_record(tmp_path):
    """the first 171 bytes: the same field names at the same offsets in the header, the ctypes views and the dtypes; the fields behind them start at byte 171"""
    head = ("leaf_count", "leaf_index", "leaf_split")
    assert [f for f, _ in M.MdLcu._fields_[:3]] == [f for f, _ in MM.MdcLcu._fields_[:3]] == list(head) == list(S.MD_LCU_DTYPE.names[:3]) == list(MR.MDC_LCU_DTYPE.names[:3])
    for f in head:
        assert getattr(M.MdLcu, f).offset == getattr(MM.MdcLcu, f).offset == S.MD_LCU_DTYPE.fields[f][1] == MR.MDC_LCU_DTYPE.fields[f][1]
    assert M.MdLcu.tile_left.offset == MM.MdcLcu.lcu_md_mode.offset == R.HEAD_BYTES == 171 and MM.MdcLcu.aura_status.offset == 172
    compiles(tmp_path, "c11", ["offsetof(SvtAmdMdLcu, %s) == offsetof(SvtAmdMdcLcu, %s)" % (f, f) for f in head] +
              ["offsetof(SvtAmdMdLcu, tile_left) == 171 && offsetof(SvtAmdMdcLcu, lcu_md_mode) == 171"])


def test_job_layout():
    assert M.MdCtlJob.sticky.offset == 64 and M.MdCtlJob.slice_type.offset == 72 and M.MdCtlJob.color_format_422_or_444.offset == 78
    assert M.MdCtlJob.tile_cols.offset == 80 and M.MdCtlJob.tile_rows.offset == 82 and M.MdCtlJob.pad.offset == 84


def test_bad_headers_are_refused_without_a_device(lib):
    jobs = (M.MdCtlJob * 1)()
    out = C.create_string_buffer(191)
    refused(lib, lib.svt_amd_md_controls_batch_launch(None, jobs, 1, 64, 64, out), M.ENTRY)
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_md_controls_batch_launch(fake, jobs, n, 64, 64, out), M.ENTRY, n)
    refused(lib, lib.svt_amd_md_controls_batch_launch(fake, None, 1, 64, 64, out), M.ENTRY)
    refused(lib, lib.svt_amd_md_controls_batch_launch(fake, jobs, 1, 64, 64, None), M.ENTRY)
    refused(lib, lib.svt_amd_md_controls_batch_launch(fake, jobs, 1, 8256, 8192, out), M.ENTRY, "more than 16,384 LCUs")   # 129 x 128; the context is not read yet
    refused_as(lib, lib.svt_amd_md_controls_batch_launch(fake, jobs, 1, 0, 64, out), M.ENTRY + ": job 0: a picture of 0x64 (at most 16384 LCUs)")
    refused_as(lib, lib.svt_amd_md_controls_batch_launch(fake, jobs, 1, 16384, 16384, out), M.ENTRY + ": job 0: a picture of 16384x16384 (at most 16384 LCUs)")
    assert lib.svt_amd_md_picture_set_controls(None, fake, out) == BAD_PARAM and lib.svt_amd_md_picture_set_controls(fake, None, out) == BAD_PARAM
    assert lib.svt_amd_debug_md_controls_check(None, out, 1, 0, 0, out) == BAD_PARAM


@pytest.mark.parametrize("w,h", [(64, 64), (416, 240), (2112, 1152), (3840, 2160)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h):
    assert lib.svt_amd_md_controls_bytes(w, h, M.MDCTL_LCU) == S.lcu_count(w, h) * 191
    for which in (-1, 1, 99):
        assert lib.svt_amd_md_controls_bytes(w, h, which) == 0
