"""CPU-only: the C-ABI of the stream-ordered entropy hand-off (include/svt_hevc_amd.h "Entropy hand-off pre-scan") - the entries are exported, the header and the
ctypes views (tests/handofflib.py) agree on sizes and on every offset, svt_amd_entropy_handoff_bytes is the documented arithmetic and the checks that need no
device answer without one - those of the blocking svt_amd_coeff_scan_picture, which runs the same kernels, among them."""
import ctypes as C

import numpy as np
import pytest

import handoff_numpy as N
import handofflib as H
import svtlib as S
from abi_util import compiles, exported, open_library, view_matches_dtype
from pa_batch_util import refused

VIEWS = (("SvtAmdEntropyHandoffHead", H.Head), ("SvtAmdEntropyHandoffJob", H.Job), ("SvtAmdEntropyHandoffOut", H.Out))
ENTRIES = {"svt_amd_entropy_handoff_bytes", "svt_amd_entropy_handoff_launch", "svt_amd_encdec_picture_entropy_handoff", "svt_amd_coeff_scan_picture"}


@pytest.fixture(scope="module")
def lib():
    return open_library(H.declare)


def test_entries_are_exported():
    assert ENTRIES <= exported(), ENTRIES - exported()


@pytest.mark.parametrize("std", ["c99", "c11"])
def test_structures_as_a_c_compiler_sees_the_header(tmp_path, std):
    """sizes, every offset and the constants, against the ctypes views"""
    assert (C.sizeof(H.Head), C.sizeof(H.Job), C.sizeof(H.Out)) == (32, 48, 48)
    checks = ["sizeof(%s) == %d" % (name, C.sizeof(view)) for name, view in VIEWS]
    checks += ["offsetof(%s, %s) == %d" % (name, f, getattr(view, f).offset) for name, view in VIEWS for f, _ in view._fields_]
    checks += ["SVT_AMD_ENTROPY_HANDOFF_%s == %d" % (n, v) for n, v in (("HEAD", H.HEAD), ("LCUS", H.LCUS), ("GROUPS", H.GROUPS), ("LEVELS", H.LEVELS),
                                                                      ("WORK_HEADS", H.WORK_HEADS), ("RESULT_HEADS", H.RESULT_HEADS))]
    checks += ["SVT_AMD_MDCTL_MAX_LCUS == %d" % H.MAX_LCUS, "sizeof(SvtAmdCoeffScanLcu) == %d" % H.LCU_BYTES, "sizeof(SvtAmdCoeffScanGroup) == 8",
               "sizeof(SvtAmdLcuCuResult) * SVT_AMD_LCU_MAX_CUS == %d" % H.RESULT_HEAD_BYTES]
    for wide in ("", "16"):
        checks += ["offsetof(SvtAmdLcuWork%s, src_y) == %d" % (wide, H.WORK_HEAD_BYTES), "offsetof(SvtAmdLcuResult%s, coeff_y) == %d" % (wide, H.RESULT_HEAD_BYTES),
                   "offsetof(SvtAmdLcuResult%s, rec_y) == %d" % (wide, H.RESULT_MIN_BYTES)]
    compiles(tmp_path, std, checks)


def test_the_head_view_has_the_dtypes_offsets():
    view_matches_dtype(H.Head, H.HEAD_DTYPE)


@pytest.mark.parametrize("w,h", [(64, 64), (72, 72), (200, 136), (3840, 2160)])
def test_bytes_are_the_documented_sizes(lib, w, h):
    n = S.lcu_count(w, h)
    want = {H.HEAD: 32, H.LCUS: n * 1552, H.GROUPS: n * 384 * 8, H.LEVELS: n * 6144 * 2, H.WORK_HEADS: n * 1584, H.RESULT_HEADS: n * 768}
    for which, size in want.items():
        assert lib.svt_amd_entropy_handoff_bytes(w, h, which) == size, which
    for which in (-1, 6, 99):
        assert lib.svt_amd_entropy_handoff_bytes(w, h, which) == 0
    assert lib.svt_amd_entropy_handoff_bytes(0, h, H.LCUS) == 0 and lib.svt_amd_entropy_handoff_bytes(w, 0, H.LCUS) == 0


def test_bad_calls_are_refused_without_a_device(lib):
    fake = C.create_string_buffer(1 << 16)        # stands for a context / a picture object / device memory: refused before any of them is read
    base = (C.addressof(fake) + 63) & ~63

    def good_job(**kw):
        j = H.job(base, S.LCU_WORK_DTYPE.itemsize, base, S.LCU_RESULT_DTYPE.itemsize, 4, 16, 16)
        for f, v in kw.items():
            setattr(j, f, v)
        return j

    def good_out(**kw):
        o = H.Out()
        o.head, o.lcus, o.groups, o.levels, o.work_heads, o.result_heads = base, base + 64, base + 128, base + 192, base + 256, base + 320
        for f, v in kw.items():
            setattr(o, f, v)
        return o

    j, o = good_job(), good_out()
    refused(lib, lib.svt_amd_entropy_handoff_launch(None, C.byref(j), C.byref(o)), H.ENTRY, "no context")
    refused(lib, lib.svt_amd_entropy_handoff_launch(fake, None, C.byref(o)), H.ENTRY, "no job")
    refused(lib, lib.svt_amd_entropy_handoff_launch(fake, C.byref(j), None), H.ENTRY, "no outputs")
    bad_jobs = [("no works", good_job(d_works=None)), ("no results", good_job(d_results=None)), ("works off a word", good_job(d_works=base + 2)),
                ("results off a word", good_job(d_results=base + 2)), ("work stride below the unit list", good_job(work_stride=H.WORK_HEAD_BYTES - 4)),
                ("work stride no multiple of 4", good_job(work_stride=S.LCU_WORK_DTYPE.itemsize + 2)),
                ("result stride below the coefficients", good_job(result_stride=H.RESULT_MIN_BYTES - 4)), ("result stride of the heads", good_job(result_stride=H.RESULT_HEAD_BYTES)),
                ("result stride no multiple of 4", good_job(result_stride=S.LCU_RESULT_DTYPE.itemsize + 2)), ("no LCU", good_job(n_lcus=0)),
                ("too many LCUs", good_job(n_lcus=H.MAX_LCUS + 1)), ("pad", good_job(pad=1))]
    for tag, bj in bad_jobs:
        refused(lib, lib.svt_amd_entropy_handoff_launch(fake, C.byref(bj), C.byref(o)), H.ENTRY, tag)
    bad_outs = [("no head", good_out(head=None)), ("no lcus", good_out(lcus=None)), ("no groups", good_out(groups=None)), ("no levels", good_out(levels=None)),
                ("head off a word", good_out(head=base + 2)), ("lcus off a word", good_out(lcus=base + 66)), ("groups at 4 mod 8", good_out(groups=base + 132)),
                ("levels at an odd byte", good_out(levels=base + 193)), ("work heads off a word", good_out(work_heads=base + 258)),
                ("result heads off a word", good_out(result_heads=base + 322))]
    for tag, bo in bad_outs:
        refused(lib, lib.svt_amd_entropy_handoff_launch(fake, C.byref(j), C.byref(bo)), H.ENTRY, tag)
        refused(lib, lib.svt_amd_encdec_picture_entropy_handoff(fake, fake, 16, 16, C.byref(bo)), H.PICTURE_ENTRY, tag)
    refused(lib, lib.svt_amd_encdec_picture_entropy_handoff(None, fake, 16, 16, C.byref(o)), H.PICTURE_ENTRY, "no context")
    refused(lib, lib.svt_amd_encdec_picture_entropy_handoff(fake, None, 16, 16, C.byref(o)), H.PICTURE_ENTRY, "no picture object")
    refused(lib, lib.svt_amd_encdec_picture_entropy_handoff(fake, fake, 16, 16, None), H.PICTURE_ENTRY, "no outputs")


def test_the_blocking_entry_refuses_bad_calls_without_a_device(lib):
    """the first check keeps its text, whichever parameter it meets; device arrays the kernels could not read by words are refused in a text that names the entry"""
    fake = C.create_string_buffer(1 << 16)        # stands for the context, the records and the outputs: refused before any of them is read
    base = (C.addressof(fake) + 63) & ~63
    good = dict(ctx=base, works=base + 64, work_stride=S.LCU_WORK_DTYPE.itemsize, results=base + 128, result_stride=S.LCU_RESULT_DTYPE.itemsize, device_arrays=0,
                n_lcus=4, lcus=base + 192, groups=base + 256, group_capacity=16, levels=base + 320, level_capacity=16, totals=C.cast(base + 384, C.POINTER(H.u32 * 2)))

    def call(**kw):
        return lib.svt_amd_coeff_scan_picture(*{**good, **kw}.values())

    bad = [(p, {p: None}) for p in ("ctx", "works", "results", "lcus", "groups", "levels", "totals")]
    bad += [("no LCU", dict(n_lcus=0)), ("work stride below the unit list", dict(work_stride=H.WORK_HEAD_BYTES - 1)),
            ("result stride below the coefficients", dict(result_stride=H.RESULT_MIN_BYTES - 1))]
    for device_arrays in (0, 1):
        for tag, kw in bad:
            rc = call(device_arrays=device_arrays, **kw)
            assert rc == -1 and lib.svt_amd_last_error() == b"svt_amd_coeff_scan_picture: bad parameter", (tag, rc, lib.svt_amd_last_error())
    for tag, kw in (("works at an odd byte", dict(works=base + 65)), ("results at an odd byte", dict(results=base + 129)), ("results off a word", dict(results=base + 130)),
                    ("work stride no multiple of 4", dict(work_stride=S.LCU_WORK_DTYPE.itemsize + 2)),
                    ("result stride no multiple of 4", dict(result_stride=S.LCU_RESULT_DTYPE.itemsize + 2))):
        refused(lib, call(device_arrays=1, **kw), H.BLOCKING_ENTRY, tag)
        assert b"4-byte aligned" in lib.svt_amd_last_error(), tag


def works_of(units):
    w = np.zeros(1, S.LCU_WORK_DTYPE)
    w["num_cus"] = len(units)
    for c, (x, y, s) in enumerate(units[:64]):
        w["cu"][0][c]["x"], w["cu"][0][c]["y"], w["cu"][0][c]["size"] = x, y, s
    return w


def test_the_restated_rules():
    """the numpy restatement on hand-made unit lists: what it refuses and what it counts"""
    quad = [(0, 0, 32), (32, 0, 32), (0, 32, 32), (32, 32, 32)]
    assert N.lcu_status(works_of(quad)[0]) == (False, 0) and N.lcu_status(works_of([(0, 0, 64)])[0]) == (False, 0)
    for bad in ((0, 0, 12), (60, 0, 16), (0, 4, 8), (32, 0, 64), (0, 0, 0)):
        assert N.lcu_status(works_of([bad])[0]) == (False, 1), bad
    assert N.lcu_status(works_of([(0, 0, 64), (0, 0, 8)])[0]) == (False, 1)
    assert N.bad_slots(works_of([(32, 0, 64)])[0]) == [0, 1, 2, 3, 4] and N.bad_slots(works_of([(0, 0, 64), (0, 0, 8)])[0]) == [0]
    assert N.lcu_status(works_of(quad + [(0, 0, 8)])[0]) == (True, 0)          # well-formed units that overlap
    long_list = works_of(quad)
    long_list["num_cus"] = 65
    assert N.lcu_status(long_list[0]) == (True, 0) and N.bad_slots(long_list[0]) == list(range(64))
    many = np.concatenate([works_of(quad), long_list, works_of([(0, 0, 12), (8, 8, 8), (3, 0, 8)]), works_of([(0, 0, 64)])])
    assert N.check(many) == {"bad_lcus": 1, "first_bad_lcu": 1, "bad_units": 2, "first_bad_unit_lcu": 2}
    assert N.check(many[:1]) == {"bad_lcus": 0, "first_bad_lcu": N.NONE, "bad_units": 0, "first_bad_unit_lcu": N.NONE}


def test_every_recorded_unit_tree_is_well_formed():
    """the rules refuse nothing the blocking entry is tested on: every LCU of every recorded encode"""
    from test_oracle_encodepass_golden import ALL, load_case
    lcus = units = 0
    for name in ALL:
        g, _, _ = load_case(name)
        assert N.check(g["work"]) == {"bad_lcus": 0, "first_bad_lcu": N.NONE, "bad_units": 0, "first_bad_unit_lcu": N.NONE}, name
        lcus, units = lcus + len(g["work"]), units + int(g["work"]["num_cus"].sum())
    assert len(ALL) == 36 and (lcus, units) == (1562, 8871)
