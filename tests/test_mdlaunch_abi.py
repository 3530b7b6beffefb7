"""CPU-only: the C-ABI of the stream-ordered mode-decision launch (include/svt_hevc_amd.h: svt_amd_md_encode_picture_launch, svt_amd_encdec_picture_md_records) -
both entries are exported, the header and the ctypes views (tests/mdlaunchlib.py) agree on sizes and on every offset, and every check that needs no device refuses
without one, in the entry's name."""
import ctypes as C
import os

import numpy as np
import pytest

import mdlaunchlib as M
import svtlib as S
from abi_util import compiles, exported, open_library
from pa_batch_util import BAD_PARAM, refused

VIEWS = (("SvtAmdMdLaunchJob", M.LaunchJob), ("SvtAmdMdLaunchStatus", M.LaunchStatus), ("SvtAmdMdCtlCheck", M.CtlCheck))


@pytest.fixture(scope="module")
def lib():
    return open_library(M.declare)


def test_entries_are_exported():
    assert {M.ENTRY, M.RECORDS_ENTRY} <= exported()


def test_structure_sizes_and_offsets_in_c99(tmp_path):
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS]
    checks += ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_]
    checks += ["SVT_AMD_MD_LAUNCH_DECIDE_ONLY == %d" % M.DECIDE_ONLY]
    compiles(tmp_path, "c99", checks)


def test_bad_launches_are_refused_without_a_device(lib):
    """a zeroed block stands for the context, the picture object (no size, no sample width, nothing bound) and device memory: every rule below is judged before any of
    them is used, and nothing is written to the block but the binding the test itself sets"""
    fake = C.create_string_buffer(8192)
    a = C.addressof(fake)
    gi = np.load(os.path.join(S.GOLDEN_DIR, "md_i_xc_binary_192x128_m9_q0.npz"))
    gb = np.load(os.path.join(S.GOLDEN_DIR, "md_b_xc_whiteblack_192x128_m8_q0.npz"))
    P, PB, X = np.ascontiguousarray(gi["pic"][0:1]), np.ascontiguousarray(gb["pic"][0:1]), np.ascontiguousarray(gb["inter"][0:1])
    cost = np.ascontiguousarray(gi["cost"][0])

    def good(inter=False):
        j = M.LaunchJob()
        j.P, j.X, j.cost, j.d_lcus = (PB if inter else P).ctypes.data, X.ctypes.data if inter else None, cost.ctypes.data, a
        j.d_src[0], j.d_src[1], j.d_src[2] = a, a + 4, a + 8
        j.src_pitch_y, j.src_pitch_c, j.d_ois, j.d_me, j.d_tmvp, j.tiles = 192, 96, a, a, a, 1
        return j

    def bad(what, text, change=None, inter=False, ctx=fake, pic=fake, status=None, job=True):
        j = good(inter)
        if change:
            change(j)
        refused(lib, lib.svt_amd_md_encode_picture_launch(ctx, pic, C.byref(j) if job else None, status), M.ENTRY, what)
        assert text in lib.svt_amd_last_error(), (what, lib.svt_amd_last_error())

    def setter(field, value):
        return lambda j: setattr(j, field, value)

    def item(field, k, value):
        def change(j):
            getattr(j, field)[k] = value
        return change

    bad("no context", b"a context", ctx=None)
    bad("no picture object", b"a context", pic=None)
    bad("no job", b"a context", job=False)
    for k in range(2):
        bad("pad[%d]" % k, b"pad word", item("pad", k, 1))
    for flags in (2, 0x80000000, 3):
        bad("flags %x" % flags, b"unknown flags", setter("flags", flags))
    bad("no picture controls", b"picture controls", setter("P", None))
    bad("no controls array", b"LCU controls", setter("d_lcus", None))
    for k in range(3):
        bad("no plane %d" % k, b"source planes", item("d_src", k, None))
    bad("decisions only of an I picture", b"DECIDE_ONLY", setter("flags", M.DECIDE_ONLY))
    for k in range(3):
        for off in (1, 2, 3):
            bad("plane %d at byte %d" % (k, off), b"4-byte aligned", item("d_src", k, a + off))
    bad("a status record at an odd address", b"4-byte aligned", status=C.c_void_p(a + 2))
    bad("luma pitch below the width", b"below the plane widths", setter("src_pitch_y", 188))
    bad("chroma pitch below the width", b"below the plane widths", setter("src_pitch_c", 92))
    unsupported = P.copy()
    unsupported["chroma_level"] = 0
    assert lib.svt_amd_md_picture_supported(unsupported.ctypes.data) == 0 and lib.svt_amd_md_picture_supported(P.ctypes.data) == 1
    bad("a picture the revision does not cover", b"svt_amd_md_picture_supported", setter("P", unsupported.ctypes.data))
    bad("not the object's size", b"not the picture object's size")                          # the zeroed object is 0 x 0
    bad("a P / B picture, not the object's size", b"not the picture object's size", inter=True)
    # a binding that waits for a blocking call: consumed, refused, and gone
    for bind in (lib.svt_amd_md_picture_set_controls, lib.svt_amd_md_picture_set_motion_field):
        assert bind(fake, fake, C.c_void_p(a + 4096)) == 0
        assert fake.raw != bytes(8192)
        bad("a pending binding", b"is bound to the picture object")
        assert fake.raw == bytes(8192)                                                      # dropped, and nothing else was written
        bad("... which is gone", b"not the picture object's size")
    assert fake.raw == bytes(8192)


def test_records_of_nothing_are_refused(lib):
    fake = C.create_string_buffer(8192)                                                    # an object no mode-decision call has touched
    out = C.c_void_p(1)
    for pic in (None, fake):
        rc = lib.svt_amd_encdec_picture_md_records(pic, C.byref(out), None, None, None, None)
        refused(lib, rc, M.RECORDS_ENTRY, pic)
    assert out.value == 1
