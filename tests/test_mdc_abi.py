"""CPU-only: the C-ABI of the batched mode-decision configuration (include/svt_hevc_amd.h "Batched mode-decision configuration") - the entries are exported, the
header, the ctypes views (tests/mdclib.py) and the numpy layouts (tests/mdc_records.py) agree on sizes and offsets, the checks that need no device answer
without one, and svt_amd_md_config_bytes is the documented arithmetic."""
import ctypes as C

import pytest

import mdc_records as R
import mdclib as M
import svtlib as S
from abi_util import compiles, exported, open_library, view_matches_dtype
from pa_batch_util import refused, refused_as


@pytest.fixture(scope="module")
def lib():
    return open_library(M.declare)


def test_entries_are_exported():
    assert {"svt_amd_md_config_batch_launch", "svt_amd_md_config_bytes"} <= exported()


def test_structure_sizes_in_c99(tmp_path):
    """sizeof of the three structures (and of the table) as a C99 compiler sees the header, against the numpy layouts"""
    assert R.MDC_LCU_DTYPE.itemsize == 184 and R.MDC_PIC_DTYPE.itemsize == 48
    checks = ["sizeof(SvtAmdMdcJob) == %d" % C.sizeof(M.MdcJob), "sizeof(SvtAmdMdcLcu) == %d" % R.MDC_LCU_DTYPE.itemsize,
              "sizeof(SvtAmdMdcPic) == %d" % R.MDC_PIC_DTYPE.itemsize, "sizeof(SvtAmdMdcArrays) == 2 * sizeof(void *)", "SVT_AMD_MDC_LCU == 0 && SVT_AMD_MDC_PICTURE == 1",
              "SVT_AMD_MDC_MAX_LCUS == %d" % M.MAX_LCUS]
    compiles(tmp_path, "c99", checks)


def test_header_offsets_field_by_field(tmp_path):
    """every field of the header's three structures lies where the ctypes view has it"""
    checks = ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in (("SvtAmdMdcJob", M.MdcJob), ("SvtAmdMdcLcu", M.MdcLcu), ("SvtAmdMdcPic", M.MdcPic))
              for f, _ in view._fields_]
    compiles(tmp_path, "c11", checks)


@pytest.mark.parametrize("view,dtype", [(M.MdcLcu, R.MDC_LCU_DTYPE), (M.MdcPic, R.MDC_PIC_DTYPE)])
def test_ctypes_views_have_the_dtypes_offsets(view, dtype):
    view_matches_dtype(view, dtype)


def test_the_lcu_record_begins_like_the_mode_decision_record():
    """the first 171 bytes: leaf_count, leaf_index[85], leaf_split[85] in the order and widths of SvtAmdMdLcu (svtlib.MD_LCU_DTYPE)"""
    md, mdc = S.MD_LCU_DTYPE, R.MDC_LCU_DTYPE
    assert md.names[:3] == mdc.names[:3] == ("leaf_count", "leaf_index", "leaf_split")
    for f in md.names[:3]:
        assert md.fields[f][:2] == mdc.fields[f][:2], f
    assert mdc.fields["lcu_md_mode"][1] == 171


def test_job_layout():
    assert C.sizeof(M.MdcJob) == 104 and M.MdcJob.cur_slot.offset == 64 and M.MdcJob.slice_type.offset == 68 and M.MdcJob.pad.offset == 91
    assert M.MdcJob.lambda_sad.offset == 92 and M.MdcJob.split_flag_bits.offset == 96


def test_bad_headers_are_refused_without_a_device(lib):
    jobs, table = (M.MdcJob * 1)(), M.MdcArrays()
    refused(lib, lib.svt_amd_md_config_batch_launch(None, jobs, 1, 64, 64, C.byref(table)), M.ENTRY)
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_md_config_batch_launch(fake, jobs, n, 64, 64, C.byref(table)), M.ENTRY, n)
    refused(lib, lib.svt_amd_md_config_batch_launch(fake, None, 1, 64, 64, C.byref(table)), M.ENTRY)
    refused(lib, lib.svt_amd_md_config_batch_launch(fake, jobs, 1, 64, 64, None), M.ENTRY)
    # ... nor for the picture's size: the bound of the kernels is tested before the context's own
    refused_as(lib, lib.svt_amd_md_config_batch_launch(fake, jobs, 1, 0, 64, C.byref(table)), M.ENTRY + ": job 0: a picture of 0x64 (at most 13854 LCUs)")
    refused_as(lib, lib.svt_amd_md_config_batch_launch(fake, jobs, 1, 7552, 7552, C.byref(table)), M.ENTRY + ": job 0: a picture of 7552x7552 (at most 13854 LCUs)")   # 118 x 118


@pytest.mark.parametrize("w,h", [(64, 64), (416, 240), (3840, 2160)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h):
    assert lib.svt_amd_md_config_bytes(w, h, M.MDC_LCU) == S.lcu_count(w, h) * R.MDC_LCU_DTYPE.itemsize
    assert lib.svt_amd_md_config_bytes(w, h, M.MDC_PICTURE) == R.MDC_PIC_DTYPE.itemsize
    for which in (-1, 2, 99):
        assert lib.svt_amd_md_config_bytes(w, h, which) == 0
