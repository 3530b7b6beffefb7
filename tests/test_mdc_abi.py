"""CPU-only: the C-ABI of the batched mode-decision configuration (include/svt_hevc_amd.h "Batched mode-decision configuration") - the entries are exported, the
header, the ctypes views (tests/mdclib.py) and the numpy layouts (tests/mdc_records.py) agree on sizes and offsets, the checks that need no device answer
without one, and svt_amd_md_config_bytes is the documented arithmetic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mdc_records as R
import mdclib as M
import svtlib as S
from pa_batch_util import refused


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(S.PRODUCT_SO), "run `python __graft_entry__.py build` first"
    return M.declare(C.CDLL(S.PRODUCT_SO))


def test_entries_are_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.PRODUCT_SO], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert {"svt_amd_md_config_batch_launch", "svt_amd_md_config_bytes"} <= exported


def test_structure_sizes_in_c99(tmp_path):
    """sizeof of the three structures (and of the table) as a C99 compiler sees the header, against the numpy layouts"""
    assert R.MDC_LCU_DTYPE.itemsize == 184 and R.MDC_PIC_DTYPE.itemsize == 48
    checks = ["sizeof(SvtAmdMdcJob) == %d" % C.sizeof(M.MdcJob), "sizeof(SvtAmdMdcLcu) == %d" % R.MDC_LCU_DTYPE.itemsize,
              "sizeof(SvtAmdMdcPic) == %d" % R.MDC_PIC_DTYPE.itemsize, "sizeof(SvtAmdMdcArrays) == 2 * sizeof(void *)", "SVT_AMD_MDC_LCU == 0 && SVT_AMD_MDC_PICTURE == 1",
              "SVT_AMD_MDC_MAX_LCUS == %d" % M.MAX_LCUS]
    src = tmp_path / "t.c"
    src.write_text('#include "svt_hevc_amd.h"\n' + "".join('_Static_assert(%s, "%s");\n' % (c, c) for c in checks) + 'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_header_offsets_field_by_field(tmp_path):
    """every field of the header's three structures lies where the ctypes view has it"""
    checks = ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in (("SvtAmdMdcJob", M.MdcJob), ("SvtAmdMdcLcu", M.MdcLcu), ("SvtAmdMdcPic", M.MdcPic))
              for f, _ in view._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "svt_hevc_amd.h"\n' + "".join('_Static_assert(%s, "%s");\n' % (c, c) for c in checks) + 'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("view,dtype", [(M.MdcLcu, R.MDC_LCU_DTYPE), (M.MdcPic, R.MDC_PIC_DTYPE)])
def test_ctypes_views_have_the_dtypes_offsets(view, dtype):
    assert C.sizeof(view) == dtype.itemsize
    assert [f for f, _ in view._fields_] == list(dtype.names)
    for f, t in view._fields_:
        sub, offset = dtype.fields[f][:2]
        assert getattr(view, f).offset == offset and C.sizeof(t) == sub.itemsize, f
        scalar = getattr(t, "_type_", t) if hasattr(t, "_length_") else t
        assert np.dtype(scalar) == sub.base.newbyteorder("="), f


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


@pytest.mark.parametrize("w,h", [(64, 64), (416, 240), (3840, 2160)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h):
    assert lib.svt_amd_md_config_bytes(w, h, M.MDC_LCU) == S.lcu_count(w, h) * R.MDC_LCU_DTYPE.itemsize
    assert lib.svt_amd_md_config_bytes(w, h, M.MDC_PICTURE) == R.MDC_PIC_DTYPE.itemsize
    for which in (-1, 2, 99):
        assert lib.svt_amd_md_config_bytes(w, h, which) == 0
