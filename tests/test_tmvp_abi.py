"""CPU-only: the C-ABI of the temporal motion field on the device (include/svt_hevc_amd.h "Temporal motion field on the device") - the entries are exported, the
header, the ctypes views (tests/tmvplib.py) and the numpy layouts agree on sizes and on every offset, svt_amd_motion_field_bytes is the documented arithmetic
and the checks that need no device answer without one."""
import ctypes as C

import pytest

import svtlib as S
import tmvplib as T
from abi_util import compiles, exported, open_library, view_matches_dtype
from pa_batch_util import BAD_PARAM, refused

VIEWS = (("SvtAmdMotionFieldJob", T.MotionFieldJob), ("SvtAmdRefStats", T.RefStats), ("SvtAmdTmvpLcu", T.TmvpLcu), ("SvtAmdLcuCu", T.LcuCu))
ENTRIES = {"svt_amd_motion_field_bytes", "svt_amd_motion_field_launch", "svt_amd_encdec_picture_motion_field", "svt_amd_md_picture_set_motion_field"}


@pytest.fixture(scope="module")
def lib():
    return open_library(T.declare)


def test_entries_are_exported():
    assert ENTRIES <= exported(), ENTRIES - exported()


def test_structure_sizes_in_c99(tmp_path):
    """sizeof of the structures as a C99 compiler sees the header (_Static_assert is gcc's extension there), against the ctypes views and the numpy layouts"""
    assert (C.sizeof(T.MotionFieldJob), C.sizeof(T.RefStats), C.sizeof(T.TmvpLcu), C.sizeof(T.LcuCu), C.sizeof(T.LcuWorkHead)) == (40, 8, 416, 24, 1584)
    assert (T.REF_STATS_DTYPE.itemsize, T.TMVP_LCU_DTYPE.itemsize, S.LCU_CU_DTYPE.itemsize, T.WORK_HEAD_DTYPE.itemsize) == (8, 416, 24, 1584)
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS]
    checks += ["SVT_AMD_MOTION_FIELD == %d" % T.FIELD, "SVT_AMD_MOTION_FIELD_STATS == %d" % T.STATS, "SVT_AMD_MDCTL_MAX_LCUS == %d" % T.MAX_LCUS,
               "sizeof(SvtAmdLcuWork) == %d" % T.WORK_BYTES, "sizeof(SvtAmdLcuWork16) == %d" % T.WORK16_BYTES]
    compiles(tmp_path, "c99", checks)


def test_header_offsets_field_by_field(tmp_path):
    """every field of the header's structures lies where the ctypes view has it; the work records of both sample widths share head and unit list"""
    checks = ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_]
    for rec in ("SvtAmdLcuWork", "SvtAmdLcuWork16"):
        checks += ["offsetof(%s, %s) == %d" % (rec, f, getattr(T.LcuWorkHead, f).offset) for f, _ in T.LcuWorkHead._fields_]
        checks += ["offsetof(%s, src_y) == %d" % (rec, T.LIST_BYTES), "offsetof(%s, cu) == %d" % (rec, T.HEAD_BYTES)]
    compiles(tmp_path, "c11", checks)


@pytest.mark.parametrize("view,dtype", [(T.RefStats, T.REF_STATS_DTYPE), (T.TmvpLcu, T.TMVP_LCU_DTYPE), (T.LcuCu, S.LCU_CU_DTYPE), (T.LcuWorkHead, T.WORK_HEAD_DTYPE)])
def test_ctypes_views_have_the_dtypes_offsets(view, dtype):
    view_matches_dtype(view, dtype)


def test_the_work_head_is_the_head_of_both_work_dtypes():
    for full in (S.LCU_WORK_DTYPE, S.LCU_WORK16_DTYPE):
        for f in T.WORK_HEAD_DTYPE.names:
            assert full.fields[f][:2] == T.WORK_HEAD_DTYPE.fields[f][:2], f
        assert full.fields["src_y"][1] == T.LIST_BYTES
    assert S.LCU_WORK16_DTYPE.itemsize == T.WORK16_BYTES


def test_field_layout():
    assert (T.TmvpLcu.mv.offset, T.TmvpLcu.ref_poc.offset, T.TmvpLcu.pred_dir.offset, T.TmvpLcu.available.offset) == (0, 128, 384, 400)
    assert (T.MotionFieldJob.work_stride.offset, T.MotionFieldJob.width.offset, T.MotionFieldJob.slice_type.offset, T.MotionFieldJob.ref_poc.offset) == (8, 16, 20, 24)


@pytest.mark.parametrize("w,h", [(64, 64), (72, 72), (200, 136), (416, 240), (3840, 2160)])
def test_bytes_are_the_documented_sizes(lib, w, h):
    assert lib.svt_amd_motion_field_bytes(w, h, T.FIELD) == (S.lcu_count(w, h) + 1) * 416
    assert lib.svt_amd_motion_field_bytes(w, h, T.STATS) == 8
    for which in (-1, 2, 99):
        assert lib.svt_amd_motion_field_bytes(w, h, which) == 0
    assert lib.svt_amd_motion_field_bytes(0, h, T.FIELD) == 0 and lib.svt_amd_motion_field_bytes(w, 0, T.FIELD) == 0


def test_bad_calls_are_refused_without_a_device(lib):
    fake = C.create_string_buffer(4096)          # stands for a context / a picture object / device memory: refused before any of them is read
    out = (C.c_uint64 * 64)()
    good = T.job(C.addressof(fake), T.WORK_BYTES, 64, 64, 0)
    refused(lib, lib.svt_amd_motion_field_launch(None, C.byref(good), out, None), T.ENTRY)
    refused(lib, lib.svt_amd_motion_field_launch(fake, None, out, None), T.ENTRY)
    refused(lib, lib.svt_amd_motion_field_launch(fake, C.byref(good), None, None), T.ENTRY)
    bad = [T.job(None, T.WORK_BYTES, 64, 64, 0), T.job(C.addressof(fake), 40, 64, 64, 0), T.job(C.addressof(fake), T.LIST_BYTES - 4, 64, 64, 0),
           T.job(C.addressof(fake), T.WORK_BYTES + 2, 64, 64, 0), T.job(C.addressof(fake) + 2, T.WORK_BYTES, 64, 64, 0), T.job(C.addressof(fake), T.WORK_BYTES, 0, 64, 0),
           T.job(C.addressof(fake), T.WORK_BYTES, 64, 0, 0), T.job(C.addressof(fake), T.WORK_BYTES, 8256, 8192, 0), T.job(C.addressof(fake), T.WORK_BYTES, 64, 64, 3)]
    padded = T.job(C.addressof(fake), T.WORK_BYTES, 64, 64, 0)
    padded.pad[1] = 1
    for k, j in enumerate(bad + [padded]):
        refused(lib, lib.svt_amd_motion_field_launch(fake, C.byref(j), out, None), T.ENTRY, k)
    refused(lib, lib.svt_amd_motion_field_launch(fake, C.byref(good), C.addressof(out) + 4, None), T.ENTRY, "field alignment")
    refused(lib, lib.svt_amd_motion_field_launch(fake, C.byref(good), out, C.addressof(out) + 2), T.ENTRY, "statistics alignment")
    poc = (C.c_uint64 * 2)(1, 2)
    refused(lib, lib.svt_amd_encdec_picture_motion_field(None, fake, 0, poc, out, None), T.PICTURE_ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_motion_field(fake, None, 0, poc, out, None), T.PICTURE_ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_motion_field(fake, fake, 0, poc, None, None), T.PICTURE_ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_motion_field(fake, fake, 3, poc, out, None), T.PICTURE_ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_motion_field(fake, fake, 0, None, out, None), T.PICTURE_ENTRY)
    refused(lib, lib.svt_amd_md_picture_set_motion_field(None, fake, out), T.BIND_ENTRY)
    refused(lib, lib.svt_amd_md_picture_set_motion_field(fake, None, out), T.BIND_ENTRY)
    assert lib.svt_amd_md_picture_set_motion_field(None, None, None) == BAD_PARAM
