"""CPU-only: the C-ABI of the picture tail on the device (include/svt_hevc_amd.h "Picture tail on the device") - the entries are exported, the header and the ctypes
views (tests/taillib.py) agree on sizes and on every offset, svt_amd_picture_tail_bytes is the documented arithmetic and the checks that need no device answer
without one."""
import ctypes as C

import pytest

import svtlib as S
import tail_numpy as N
import taillib as T
from abi_util import compiles, exported, open_library
from pa_batch_util import BAD_PARAM, refused

VIEWS = (("SvtAmdTailJob", T.TailJob), ("SvtAmdTailCheck", T.TailCheck), ("SvtAmdDeblockParams", T.DeblockParams), ("SvtAmdCuMapEntry", T.CuMapEntry))
ENTRIES = {"svt_amd_picture_tail_bytes", "svt_amd_encdec_picture_tail_launch", "svt_amd_encdec_picture_tail_warmup", "svt_amd_debug_picture_tail_maps",
           "svt_amd_encode_picture_device16", "svt_amd_encode_picture_device_inter16"}


@pytest.fixture(scope="module")
def lib():
    return open_library(T.declare)


def test_entries_are_exported():
    assert ENTRIES <= exported(), ENTRIES - exported()


def test_structure_sizes_and_offsets_in_c99(tmp_path):
    assert (C.sizeof(T.TailJob), C.sizeof(T.TailCheck), C.sizeof(T.DeblockParams), C.sizeof(T.SaoDecisionParams), C.sizeof(T.CuMapEntry)) == (168, 16, 24, 88, 12)
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS] + ["sizeof(SvtAmdSaoDecisionParams) == 88", "sizeof(SvtAmdSaoLcuParams) == 72"]
    checks += ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_]
    checks += ["offsetof(SvtAmdSaoDecisionParams, %s) == %d" % (f.rstrip("_"), getattr(T.SaoDecisionParams, f).offset) for f, _ in T.SaoDecisionParams._fields_]
    checks += ["SVT_AMD_TAIL_DEBLOCK == %d" % N.DEBLOCK, "SVT_AMD_TAIL_SAO_DECIDE == %d" % N.SAO_DECIDE, "SVT_AMD_TAIL_SAO_APPLY == %d" % N.SAO_APPLY,
               "SVT_AMD_TAIL_REFERENCE == %d" % N.REFERENCE, "SVT_AMD_TAIL_LCU_PARAMS == %d" % T.LCU_PARAMS, "SVT_AMD_TAIL_CHECK == %d" % T.CHECK,
               "offsetof(SvtAmdLcuWork, src_y) == %d" % T.LIST_BYTES, "offsetof(SvtAmdLcuWork16, src_y) == %d" % T.LIST_BYTES,
               "offsetof(SvtAmdLcuResult, coeff_y) == %d" % T.RESULT_CU_BYTES, "offsetof(SvtAmdLcuResult16, coeff_y) == %d" % T.RESULT_CU_BYTES]
    compiles(tmp_path, "c99", checks)


@pytest.mark.parametrize("w,h", [(64, 64), (136, 72), (200, 136), (3840, 2160)])
def test_bytes_are_the_documented_sizes(lib, w, h):
    assert lib.svt_amd_picture_tail_bytes(w, h, T.LCU_PARAMS) == S.lcu_count(w, h) * 72
    assert lib.svt_amd_picture_tail_bytes(w, h, T.CHECK) == 16
    for which in (-1, 2, 99):
        assert lib.svt_amd_picture_tail_bytes(w, h, which) == 0
    assert lib.svt_amd_picture_tail_bytes(0, h, T.LCU_PARAMS) == 0 and lib.svt_amd_picture_tail_bytes(w, 0, T.CHECK) == 0


def test_bad_calls_are_refused_without_a_device(lib):
    fake = C.create_string_buffer(8192)          # stands for a context, a picture object (all zero: 8-bit, nothing encoded) and device memory: refused before any is used
    a = C.addressof(fake)
    ref = S.RefPicture()
    D, SD, A, R = N.DEBLOCK, N.SAO_DECIDE, N.SAO_APPLY, N.REFERENCE

    def good(stages, **kw):
        return T.job(a, S.LCU_WORK_DTYPE.itemsize, a, S.LCU_RESULT_DTYPE.itemsize, stages, **kw)
    refused(lib, lib.svt_amd_encdec_picture_tail_launch(None, fake, C.byref(good(D)), None, None, None), T.ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_tail_launch(fake, None, C.byref(good(D)), None, None, None), T.ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_tail_launch(fake, fake, None, None, None, None), T.ENTRY)
    for stages in range(0, 18):                  # the stage rules of the restatement, bit pattern by bit pattern (the object holds no picture: every other job is refused for that)
        for has_ref in (False, True):
            j = good(stages, origin=(80, 80))
            refused(lib, lib.svt_amd_encdec_picture_tail_launch(fake, fake, C.byref(j), None, None, C.byref(ref) if has_ref else None), T.ENTRY, stages)
            why = N.stages_refused(stages, 0, has_ref, 80, 80)
            text = lib.svt_amd_last_error()
            assert (b"holds no encoded picture" in text) == (why is None), (stages, has_ref, text)
            assert (b"SVT_AMD_TAIL_SAO_APPLY needs" in text) == (why == "apply") and (b"SVT_AMD_TAIL_REFERENCE needs" in text) == (why == "reference"), (stages, text)
    for origin in ((6, 80), (80, 81), (258, 80), (0, 0)):
        refused(lib, lib.svt_amd_encdec_picture_tail_launch(fake, fake, C.byref(good(R, origin=origin)), None, None, C.byref(ref)), T.ENTRY, origin)
        assert b"SVT_AMD_TAIL_REFERENCE needs" in lib.svt_amd_last_error()
    bad = [T.job(a, S.LCU_WORK_DTYPE.itemsize, None, S.LCU_RESULT_DTYPE.itemsize, D), T.job(None, S.LCU_WORK_DTYPE.itemsize, a, S.LCU_RESULT_DTYPE.itemsize, D),
           T.job(a, S.LCU_WORK_DTYPE.itemsize - 4, a, S.LCU_RESULT_DTYPE.itemsize, D), T.job(a, S.LCU_WORK_DTYPE.itemsize + 2, a, S.LCU_RESULT_DTYPE.itemsize, D),
           T.job(a + 2, S.LCU_WORK_DTYPE.itemsize, a, S.LCU_RESULT_DTYPE.itemsize, D), T.job(a, S.LCU_WORK_DTYPE.itemsize, a, S.LCU_RESULT_DTYPE.itemsize - 4, D),
           T.job(a, S.LCU_WORK_DTYPE.itemsize, a + 1, S.LCU_RESULT_DTYPE.itemsize, SD), T.job(None, 0, None, 0, D)]
    padded = good(D)
    padded.pad = 1
    for k, j in enumerate(bad + [padded]):
        refused(lib, lib.svt_amd_encdec_picture_tail_launch(fake, fake, C.byref(j), None, None, None), T.ENTRY, k)
        assert b"holds no encoded picture" not in lib.svt_amd_last_error(), k
    assert ref.d_y is None and ref.strideY == 0                      # nothing is written on a refusal
    refused(lib, lib.svt_amd_encdec_picture_tail_warmup(None, fake, 80, 80), T.WARMUP_ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_tail_warmup(fake, None, 80, 80), T.WARMUP_ENTRY)
    refused(lib, lib.svt_amd_encdec_picture_tail_warmup(fake, fake, 80, 7), T.WARMUP_ENTRY)
    refused(lib, lib.svt_amd_debug_picture_tail_maps(None, fake, None, None, None, None, None, None, None, None), T.DEBUG_ENTRY)
    refused(lib, lib.svt_amd_debug_picture_tail_maps(fake, fake, None, None, None, None, None, None, None, None), T.DEBUG_ENTRY)
    for fn in (lib.svt_amd_encode_picture_device16, lib.svt_amd_encode_picture_device_inter16):
        extra = (1,) if fn is lib.svt_amd_encode_picture_device16 else (1, 0)
        assert fn(None, fake, fake, fake, *extra) == BAD_PARAM and fn(fake, fake, None, fake, *extra) == BAD_PARAM and fn(fake, fake, fake, None, *extra) == BAD_PARAM
        assert fn(fake, fake, fake, fake, 0, *extra[1:]) == BAD_PARAM
