"""CPU-only: the C-ABI of the batched side statistics (include/svt_hevc_amd.h "Batched side statistics") - the two entries are exported, the
Python mirrors have the C layout, the parameter checks that need no device answer without one, and svt_amd_side_stats_bytes is the numpy arithmetic."""
import ctypes as C
import os
import subprocess

import pytest

import sidelib as L
from abi_util import exported, open_library
from pa_batch_util import refused
import svtlib as S


@pytest.fixture(scope="module")
def lib():
    return open_library(L.declare)


def test_side_entries_are_exported():
    assert {"svt_amd_side_stats_batch_launch", "svt_amd_side_stats_bytes"} <= exported()


def test_structure_layouts(tmp_path):
    assert C.sizeof(L.SideJob) == 12
    assert C.sizeof(L.SideArrays) == 6 * C.sizeof(C.c_void_p)
    assert L.ZZ_DTYPE.itemsize == 8
    src = tmp_path / "t.c"
    src.write_text('#include "svt_hevc_amd.h"\n'
                   '_Static_assert(sizeof(SvtAmdSideJob) == 12, "job");\n'
                   '_Static_assert(sizeof(SvtAmdSideArrays) == 6 * sizeof(void *), "arrays");\n'
                   '_Static_assert(sizeof(SvtAmdPaLcuStats) == 256 && sizeof(SvtAmdZzLcu) == 8, "records");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_bad_parameters_are_refused_without_a_device(lib):
    jobs = L.make_jobs([(0, -1, 1, 1, 1)])
    table = L.SideArrays()
    refused(lib, lib.svt_amd_side_stats_batch_launch(None, jobs, 1, 4, 4, C.byref(table)), "svt_amd_side_stats_batch_launch")
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_side_stats_batch_launch(fake, jobs, n, 4, 4, C.byref(table)), "svt_amd_side_stats_batch_launch", n)
    refused(lib, lib.svt_amd_side_stats_batch_launch(fake, None, 1, 4, 4, C.byref(table)), "svt_amd_side_stats_batch_launch")
    refused(lib, lib.svt_amd_side_stats_batch_launch(fake, jobs, 1, 4, 4, None), "svt_amd_side_stats_batch_launch")


@pytest.mark.parametrize("w,h", [(416, 240), (1920, 1080), (3840, 2160)])
def test_bytes_per_picture_are_the_numpy_sizes(lib, w, h):
    n = S.lcu_count(w, h)
    for rw, rh in ((4, 4), (1, 1), (8, 8), (3, 5)):
        got = [lib.svt_amd_side_stats_bytes(w, h, k, rw, rh) for k in range(6)]
        assert got == [n * S.PA_LCU_STATS_DTYPE.itemsize, n * 40, n * L.ZZ_DTYPE.itemsize, rw * rh * 1024, 64, 8]
        assert got == L.numpy_sizes(w, h, rw, rh)
    for which in (-1, 6, 99):
        assert lib.svt_amd_side_stats_bytes(w, h, which, 4, 4) == 0
    for rw, rh in ((0, 4), (4, 0), (9, 8), (-1, -1)):   # more than 64 regions fit no picture's 64 bytes of averages
        assert lib.svt_amd_side_stats_bytes(w, h, L.HISTOGRAM, rw, rh) == 0
