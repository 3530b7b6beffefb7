"""CPU-only: the C-ABI of the batched source-based operations (include/svt_hevc_amd.h "Batched source-based operations") - the two entries are exported, the
Python mirrors and the header agree on sizes and offsets, the checks that need no device answer without one, and svt_amd_source_ops_bytes is the documented
arithmetic."""
import ctypes as C

import pytest

import sbo_records as R
import svtlib as S
from abi_util import compiles, exported, open_library
from pa_batch_util import refused, refused_as


@pytest.fixture(scope="module")
def lib():
    return open_library(R.declare)


def test_entries_are_exported():
    assert {"svt_amd_source_ops_batch_launch", "svt_amd_source_ops_bytes"} <= exported()


def test_structure_layouts(tmp_path):
    assert C.sizeof(R.SboJob) == 208 and C.sizeof(R.SboArrays) == 2 * C.sizeof(C.c_void_p)
    assert R.SboJob.zz.offset == 40 and R.SboJob.me.offset == 176 and R.SboJob.cur_slot.offset == 192 and R.SboJob.zz_count.offset == 196
    assert R.SboJob.want_qpm.offset == 203
    lcu, pic = R.SBO_LCU_DTYPE, R.SBO_PIC_DTYPE
    assert lcu.itemsize == 24 and pic.itemsize == 168
    checks = ["sizeof(SvtAmdSboJob) == 208", "sizeof(SvtAmdSboLcu) == 24", "sizeof(SvtAmdSboPic) == 168", "sizeof(SvtAmdSboArrays) == 2 * sizeof(void *)",
              "offsetof(SvtAmdSboJob, zz) == 40", "offsetof(SvtAmdSboJob, me) == 176", "offsetof(SvtAmdSboJob, ois) == 184", "offsetof(SvtAmdSboJob, cur_slot) == 192",
              "offsetof(SvtAmdSboJob, zz_count) == 196", "offsetof(SvtAmdSboJob, slice_type) == 197", "offsetof(SvtAmdSboJob, temporal_layer_index) == 198",
              "offsetof(SvtAmdSboJob, is_used_as_reference) == 199", "offsetof(SvtAmdSboJob, resolution_class) == 200", "offsetof(SvtAmdSboJob, skip_ois_8x8) == 201",
              "offsetof(SvtAmdSboJob, cu8x8_mode) == 202", "offsetof(SvtAmdSboJob, want_qpm) == 203", "SVT_AMD_SBO_LCU == 0 && SVT_AMD_SBO_PICTURE == 1"]
    checks += ["offsetof(SvtAmdSboLcu, %s) == %d" % (f, lcu.fields[f][1]) for f in lcu.names]
    checks += ["offsetof(SvtAmdSboPic, %s) == %d" % (f, pic.fields[f][1]) for f in pic.names]
    compiles(tmp_path, "c11", checks)


def test_bad_headers_are_refused_without_a_device(lib):
    jobs, table = (R.SboJob * 1)(), R.SboArrays()
    refused(lib, lib.svt_amd_source_ops_batch_launch(None, jobs, 1, 64, 64, 1, 1, C.byref(table)), R.ENTRY)
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_source_ops_batch_launch(fake, jobs, n, 64, 64, 1, 1, C.byref(table)), R.ENTRY, n)
    refused(lib, lib.svt_amd_source_ops_batch_launch(fake, None, 1, 64, 64, 1, 1, C.byref(table)), R.ENTRY)
    refused(lib, lib.svt_amd_source_ops_batch_launch(fake, jobs, 1, 64, 64, 1, 1, None), R.ENTRY)
    # ... nor for the picture's size: the bound of the kernels is tested before the context's own
    refused_as(lib, lib.svt_amd_source_ops_batch_launch(fake, jobs, 1, 0, 64, 1, 1, C.byref(table)), R.ENTRY + ": job 0: a picture of 0x64 (at most 16384 LCUs)")
    refused_as(lib, lib.svt_amd_source_ops_batch_launch(fake, jobs, 1, 16384, 16384, 1, 1, C.byref(table)),
               R.ENTRY + ": job 0: a picture of 16384x16384 (at most 16384 LCUs)")


@pytest.mark.parametrize("w,h", [(48, 40), (64, 64), (416, 240), (704, 640), (1920, 1080), (3840, 2160)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h):
    assert lib.svt_amd_source_ops_bytes(w, h, R.SBO_LCU) == S.lcu_count(w, h) * R.SBO_LCU_DTYPE.itemsize
    assert lib.svt_amd_source_ops_bytes(w, h, R.SBO_PICTURE) == R.SBO_PIC_DTYPE.itemsize
    for which in (-1, 2, 99):
        assert lib.svt_amd_source_ops_bytes(w, h, which) == 0
