"""GPU: the entropy hand-off as a stream-ordered launch on the records in HBM (svt-hevc_amd/csrc/handoff_kernels.hip; include/svt_hevc_amd.h "Entropy hand-off
pre-scan": svt_amd_entropy_handoff_launch, svt_amd_encdec_picture_entropy_handoff) - against the CPU checker LCU by LCU, which is the proof of the one device chain,
and byte for byte against the blocking svt_amd_coeff_scan_picture, the chain's other caller, on every recorded encode; the base kernel across its chunks of 1024 LCUs; capacities that do not fit; records the host never validated;
the object form behind the launch chain without a wait; two launches in flight.  10 bits a sample: the p10_ / b10_ / i10_ recorded encodes of case 1 and the
10-bit object of case 5."""
import ctypes as C

import numpy as np
import pytest

import handoff_numpy as N
import handofflib as H
import mdlaunchlib as M
import svtlib as S
import taillib
from pa_batch_util import DeviceBuffer, is_sentinel, ok, refused
from test_oracle_encodepass_golden import ALL, load_case

pytestmark = pytest.mark.gpu
vp, u32 = C.c_void_p, C.c_uint32
MARGIN = 128 * 1024                    # the test's own memory on either side of malformed records
NOTHING = np.array([(0, -1, 0, 0, 0, 0, 0)], S.COEFF_SCAN_TU_DTYPE)[0]
EXPECTED = {}                          # fixture name -> the checker's lists of every LCU, computed once


@pytest.fixture(scope="module")
def lib(product):
    return H.declare(product)


def oracle_scan(oracle, work, res):
    oracle.svt_oracle_coeff_scan_lcu.restype, oracle.svt_oracle_coeff_scan_lcu.argtypes = C.c_int, [vp, vp, vp, vp, vp]
    lcu = np.zeros(1, S.COEFF_SCAN_LCU_DTYPE)
    groups, levels = np.zeros(H.MAX_GROUPS, S.COEFF_SCAN_GROUP_DTYPE), np.zeros(H.MAX_LEVELS, np.uint16)
    oracle.svt_oracle_coeff_scan_lcu(work.ctypes.data, res.ctypes.data, lcu.ctypes.data, groups.ctypes.data, levels.ctypes.data)
    ng, nl = int(lcu[0]["groups"]), int(lcu[0]["levels"])
    return lcu[0], groups[:ng].copy(), levels[:nl].copy()


def expected_of(oracle, works, results):
    """the checker on every record: [(SvtAmdCoeffScanLcu with bases 0, groups, levels)]"""
    return [oracle_scan(oracle, works[k:k + 1], results[k:k + 1]) for k in range(len(works))]


def fixture(oracle, name):
    """(works, results, the checker's lists) of a recorded encode; the checker runs once a fixture"""
    g, _, _ = load_case(name)
    works = np.ascontiguousarray(g["work"])
    wide = works.dtype.itemsize == S.LCU_WORK16_DTYPE.itemsize
    results = np.ascontiguousarray(g["result"]).view(S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE)
    if name not in EXPECTED:
        EXPECTED[name] = expected_of(oracle, works, results)
    return works, results, EXPECTED[name]


def totals_of(exp):
    return sum(int(e[0]["groups"]) for e in exp), sum(int(e[0]["levels"]) for e in exp)


def compare(tag, exp, got, which=None, lists=(True, True)):
    """lcus[] against the checker with the bases as exclusive sums; of the LCUs in `which` (all by default) the records and - where `lists` says the list fitted - the
    lists at their picture offsets"""
    lcus = got["lcus"]
    assert np.array_equal(lcus["groups"], [int(e[0]["groups"]) for e in exp]) and np.array_equal(lcus["levels"], [int(e[0]["levels"]) for e in exp]), tag
    assert np.array_equal(lcus["group_base"], N.exclusive_sums(lcus["groups"])) and np.array_equal(lcus["level_base"], N.exclusive_sums(lcus["levels"])), tag
    assert not lcus["pad"].any(), tag
    for k in (range(len(exp)) if which is None else which):
        want, wg, wl = exp[k]
        assert np.array_equal(lcus[k]["tu"], want["tu"]), (tag, k, np.argwhere(lcus[k]["tu"] != want["tu"])[:4].tolist())
        gb, lb = int(lcus[k]["group_base"]), int(lcus[k]["level_base"])
        if lists[0]:
            assert np.array_equal(got["groups"][gb:gb + len(wg)], wg), (tag, k, "groups")
        if lists[1]:
            assert np.array_equal(got["levels"][lb:lb + len(wl)], wl), (tag, k, "levels")


def clean_head(head, totals, overflow=0):
    assert (int(head["groups"]), int(head["levels"]), int(head["overflow"]), int(head["pad"])) == (totals[0], totals[1], overflow, 0), head
    assert (int(head["bad_lcus"]), int(head["first_bad_lcu"]), int(head["bad_units"]), int(head["first_bad_unit_lcu"])) == (0, H.NONE, 0, H.NONE), head


class Records:
    """work and result records in ONE device allocation, `margin` bytes of the test's own on either side of each array; tight: only the bytes the hand-off may
    read of a record (head and unit list; cbf / count records and coefficients), at those strides"""

    def __init__(self, lib, ctx, works, results, tight=False, margin=256):
        wb = np.ascontiguousarray(works).view(np.uint8).reshape(len(works), -1)
        rb = np.ascontiguousarray(results).view(np.uint8).reshape(len(results), -1)
        if tight:
            wb, rb = np.ascontiguousarray(wb[:, :H.WORK_HEAD_BYTES]), np.ascontiguousarray(rb[:, :H.RESULT_MIN_BYTES])
        self.n, self.work_stride, self.result_stride = len(wb), wb.shape[1], rb.shape[1]
        self.keep = (wb.reshape(-1), rb.reshape(-1))
        at_w = margin
        at_r = (at_w + wb.size + margin + 255) & ~255
        self.dev = DeviceBuffer(lib, ctx, at_r + rb.size + margin)
        self.dev.put(self.keep[0], at_w)
        self.dev.put(self.keep[1], at_r)
        self.d_works, self.d_results = self.dev.at(at_w), self.dev.at(at_r)

    def job(self, gcap, lcap):
        return H.job(self.d_works, self.work_stride, self.d_results, self.result_stride, self.n, gcap, lcap)

    def free(self):
        self.dev.free()


def launch(lib, ctx, recs, out):
    return lib.svt_amd_entropy_handoff_launch(ctx, C.byref(recs.job(out.gcap, out.lcap)), C.byref(out.out))


def blocking(lib, ctx, recs):
    """svt_amd_coeff_scan_picture on the same device arrays, worst-case capacities: the other caller of the launch's kernels, with a host half of its own (scratch
    carve, clamped capacities, downloads)"""
    n = recs.n
    lcus, groups, levels = np.zeros(n, S.COEFF_SCAN_LCU_DTYPE), np.zeros(H.MAX_GROUPS * n, S.COEFF_SCAN_GROUP_DTYPE), np.zeros(H.MAX_LEVELS * n, np.uint16)
    totals = (u32 * 2)()
    ok(lib, lib.svt_amd_coeff_scan_picture(ctx, vp(recs.d_works), recs.work_stride, vp(recs.d_results), recs.result_stride, 1, n, lcus.ctypes.data, groups.ctypes.data,
                                           len(groups), levels.ctypes.data, len(levels), C.byref(totals)))
    return lcus, groups, levels, (int(totals[0]), int(totals[1]))


# ---- 1. every recorded encode -----------------------------------------------------------------------------------------------------------------------------

def test_the_recorded_encodes_cover_what_case_one_claims(oracle):
    """both sample widths, LCUs without a group and with the worst case of 384, all three scans, 64x64 units: by the fixtures and the checker alone"""
    assert len(ALL) == 36
    wide = lone64 = 0
    groups, scans = set(), set()
    for name in ALL:
        works, results, exp = fixture(oracle, name)
        assert 6 <= len(works) <= 200, name
        wide += works.dtype.itemsize == S.LCU_WORK16_DTYPE.itemsize
        lone64 += int(((works["num_cus"] == 1) & (works["cu"]["size"][:, 0] == 64)).sum())
        for e in exp:
            groups.add(int(e[0]["groups"]))
            coded = e[0]["tu"]["last_scan_set"] >= 0
            scans |= set(e[0]["tu"]["scan_index"][coded & (e[0]["tu"]["dc_only"] == 0)].tolist())
    assert wide and lone64 and {0, H.MAX_GROUPS} <= groups and scans == {0, 1, 2}


@pytest.mark.parametrize("name", ALL)
def test_recorded_pictures_match_the_checker_and_the_blocking_entry(lib, oracle, gpu_ctx, name):
    """the records uploaded at their full strides; a first launch at the worst-case capacities, then one at the exact fit {head.groups, head.levels}: the checker
    LCU by LCU - the proof of the chain both entries run -, the head copies, a clean head, every sentinel intact; and the blocking entry's bytes on the same device
    arrays: the same kernels from another host half, so equal bytes say that the two host halves agree (arrays, capacities, what is downloaded), not that the chain
    is right"""
    works, results, exp = fixture(oracle, name)
    n, totals = len(works), totals_of(exp)
    recs = Records(lib, gpu_ctx, works, results)
    wide, fit = H.Outputs(lib, gpu_ctx, n, H.MAX_GROUPS * n, H.MAX_LEVELS * n), H.Outputs(lib, gpu_ctx, n, totals[0], totals[1])
    try:
        ok(lib, launch(lib, gpu_ctx, recs, wide))
        ok(lib, launch(lib, gpu_ctx, recs, fit))
        first, got = wide.get(), fit.get()
        for g in (first, got):
            clean_head(g["head"], totals)
            compare(name, exp, g)
        assert is_sentinel(first["raw"]["groups"][8 * totals[0]:]) and is_sentinel(first["raw"]["levels"][2 * totals[1]:]), name
        b_lcus, b_groups, b_levels, b_totals = blocking(lib, gpu_ctx, recs)
        assert b_totals == totals and got["lcus"].tobytes() == b_lcus.tobytes(), name
        assert got["groups"].tobytes() == b_groups[:totals[0]].tobytes() and got["levels"].tobytes() == b_levels[:totals[1]].tobytes(), name
        wh, rh = N.head_copies(works, results)
        assert np.array_equal(got["work_heads"], wh) and np.array_equal(got["result_heads"], rh), name
    finally:
        for o in (recs, wide, fit):
            o.free()


# ---- 2. the base kernel across its chunks -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 1024, 1025, 2049])
def test_bases_across_the_chunks_of_the_base_kernel(lib, oracle, gpu_ctx, n):
    """the 12 records of one picture repeated, at the smallest strides the entry takes: bases = exclusive sums of the checker's counts; the lists of the first, the
    last and every 97th LCU"""
    works, results, exp12 = fixture(oracle, "i_noise_200x136_m6")
    assert len(works) == 12
    idx = np.arange(n) % 12
    exp = [exp12[k] for k in idx]
    totals = totals_of(exp)
    recs = Records(lib, gpu_ctx, works[idx], results[idx], tight=True)
    out = H.Outputs(lib, gpu_ctx, n, totals[0], totals[1], heads=False)
    try:
        assert (recs.work_stride, recs.result_stride) == (H.WORK_HEAD_BYTES, H.RESULT_MIN_BYTES)
        ok(lib, launch(lib, gpu_ctx, recs, out))
        got = out.get()
        clean_head(got["head"], totals)
        compare(n, exp, got, sorted(set(range(0, n, 97)) | {0, n - 1}))
    finally:
        recs.free()
        out.free()


# ---- 3. capacities that do not fit ----------------------------------------------------------------------------------------------------------------------------

def test_overflow_is_reported_and_writes_only_what_fits(lib, oracle, gpu_ctx):
    """groups one short with exact levels, the reverse, both 0: head names what the picture needs and the list that overflowed; an LCU whose range fits has its
    list, one whose range does not has nothing written; nothing at or behind a capacity is touched; lcus[] is the fitting run's"""
    name = "sao_p_noise_320x256_m8"
    works, results, exp = fixture(oracle, name)
    n, totals = len(works), totals_of(exp)
    assert totals == (16001, 159356)
    recs = Records(lib, gpu_ctx, works, results)
    fit = H.Outputs(lib, gpu_ctx, n, totals[0], totals[1], heads=False)
    try:
        ok(lib, launch(lib, gpu_ctx, recs, fit))
        want = fit.get()
        clean_head(want["head"], totals)
        compare(name, exp, want)
        for gcap, lcap, bits in ((totals[0] - 1, totals[1], 1), (totals[0], totals[1] - 1, 2), (0, 0, 3)):
            out = H.Outputs(lib, gpu_ctx, n, gcap, lcap, heads=False)
            try:
                ok(lib, launch(lib, gpu_ctx, recs, out))
                got = out.get()                                                  # (asserts the sentinel behind every array, so at and behind the capacities)
                clean_head(got["head"], totals, bits)
                assert got["lcus"].tobytes() == want["lcus"].tobytes(), bits
                fitted = [0, 0]
                for k in range(n):
                    lc = got["lcus"][k]
                    for i, (lst, base, count, cap, size) in enumerate((("groups", "group_base", "groups", gcap, 8), ("levels", "level_base", "levels", lcap, 2))):
                        b, c = int(lc[base]), int(lc[count])
                        if b + c <= cap:
                            assert got[lst][b:b + c].tobytes() == want[lst][b:b + c].tobytes(), (bits, k, lst)
                            fitted[i] += c > 0
                        else:
                            assert is_sentinel(got["raw"][lst][size * min(b, cap):]), (bits, k, lst)
                assert (fitted[0] > 0) == (gcap > 0) and (fitted[1] > 0) == (lcap > 0), (bits, fitted)
            finally:
                out.free()
    finally:
        recs.free()
        fit.free()


# ---- 4. records the host never validated ---------------------------------------------------------------------------------------------------------------------

def test_malformed_records_are_counted_and_code_nothing(lib, oracle, gpu_ctx):
    """a recorded picture with seven records rewritten (each refused unit with cbf 1 in all three planes, so that a forgotten guard would scan it), in the middle of
    one allocation with 128 KB of the test's own memory around each array: the counts of the numpy restatement, every refused slot "nothing to code", everything else
    what the checker gives on records in which the refused slots are not coded - so the LCUs around the rewritten ones keep the untouched run's records and lists"""
    name = "sao_p_noise_320x256_m8"
    works, results, exp_good = fixture(oracle, name)
    works, results, rewritten = N.malformed(works, results)
    n, want_check = len(works), N.MALFORMED_CHECK
    exp = expected_of(oracle, *N.sanitized(works, results))
    for k in range(n):
        if k not in rewritten:
            assert exp[k][0].tobytes() == exp_good[k][0].tobytes() and exp[k][1].tobytes() == exp_good[k][1].tobytes() and exp[k][2].tobytes() == exp_good[k][2].tobytes()
    totals = totals_of(exp)
    recs = Records(lib, gpu_ctx, works, results, margin=MARGIN)
    out = H.Outputs(lib, gpu_ctx, n, totals[0], totals[1])
    try:
        ok(lib, launch(lib, gpu_ctx, recs, out))
        got = out.get()
        head = got["head"]
        assert (int(head["groups"]), int(head["levels"]), int(head["overflow"]), int(head["pad"])) == (totals[0], totals[1], 0, 0)
        assert {f: int(head[f]) for f in want_check} == want_check
        compare(name, exp, got)
        for k in rewritten:
            slots = N.bad_slots(works[k])
            assert slots and (got["lcus"][k]["tu"][:, slots] == NOTHING).all(), k
        for k in (2, 5):
            assert int(got["lcus"][k]["groups"]) == 0 and int(got["lcus"][k]["levels"]) == 0 and (got["lcus"][k]["tu"] == NOTHING).all()
        wh, rh = N.head_copies(works, results)                                 # a copy, not a judgement
        assert np.array_equal(got["work_heads"], wh) and np.array_equal(got["result_heads"], rh)
    finally:
        recs.free()
        out.free()


# ---- 5. the object form behind the launch chain ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bps", [("i_xc_binary_192x128_m9_q0", 1), ("p_objects_320x192_m8_ld", 1), ("i_motion_416x240_m9", 2)])
def test_the_object_form_behind_the_launch_chain(lib, oracle, name, bps):
    """svt_amd_md_encode_picture_launch, the tail (deblocking, NULL records) and the hand-off queued on one context with nothing in between; after ONE
    svt_amd_synchronize the hand-off equals the checker on the records downloaded through svt_amd_encdec_picture_md_records"""
    import test_gpu_picture_tail as TT
    from test_gpu_md_launch import World
    from test_gpu_mdctl_batch import _md_sig
    _md_sig(lib)
    taillib.declare(M.declare(lib))
    g = M.load(name)
    world = World(lib, g, 0, bps)
    inp = world.inputs()
    n = world.n
    slice_type = int(world.P["slice_type"][0])
    poc = (int(world.X["ref_poc"][0][0]), int(world.X["ref_poc"][0][1])) if world.inter else (0, 0)
    tail = TT.Tail(lib, world.ctx, world.pic, world.w, world.h, bps == 2, None, TT.D, slice_type, poc)
    out = H.Outputs(lib, world.ctx, n, H.MAX_GROUPS * n, H.MAX_LEVELS * n)
    try:
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, M.tiles_of(world.lcus)), inp))
        ok(lib, tail.launch())
        ok(lib, lib.svt_amd_encdec_picture_entropy_handoff(world.ctx, world.pic, out.gcap, out.lcap, C.byref(out.out)))
        ok(lib, lib.svt_amd_synchronize(world.ctx))                             # the one wait
        assert inp.status().refused == 0
        _, works_b, res_b = M.fetch(lib, world.ctx, world.pic, n, bps == 2)
        works = np.frombuffer(works_b, S.LCU_WORK16_DTYPE if bps == 2 else S.LCU_WORK_DTYPE)
        results = np.frombuffer(res_b, S.LCU_RESULT16_DTYPE if bps == 2 else S.LCU_RESULT_DTYPE)
        assert int(works["num_cus"].sum()) >= n
        exp = expected_of(oracle, works, results)
        got = out.get()
        totals = totals_of(exp)
        assert totals[1] > 0
        clean_head(got["head"], totals)
        compare((name, bps), exp, got)
        wh, rh = N.head_copies(works, results)
        assert np.array_equal(got["work_heads"], wh) and np.array_equal(got["result_heads"], rh)
    finally:
        out.free()
        tail.free()
        inp.free()
        world.free()


def test_the_object_form_is_refused_where_the_motion_field_is(lib):
    """an untouched object, a decide-only P / B call, an object with a rank rectangle: each names the entry and queues nothing - the outputs keep their sentinel
    after a synchronise; then the same arrays take the result"""
    from test_gpu_md_launch import World
    from test_gpu_mdctl_batch import Rect, _md_sig
    _md_sig(lib)
    M.declare(lib)
    lib.svt_amd_encdec_picture_set_rect.restype, lib.svt_amd_encdec_picture_set_rect.argtypes = C.c_int, [vp, vp, vp]
    world = World(lib, M.load("p_objects_320x192_m8_ld"), 0, 1)
    inp = world.inputs()
    n = world.n
    out = H.Outputs(lib, world.ctx, n, H.MAX_GROUPS * n, H.MAX_LEVELS * n)

    def handoff():
        return lib.svt_amd_encdec_picture_entropy_handoff(world.ctx, world.pic, out.gcap, out.lcap, C.byref(out.out))
    try:
        refused(lib, handoff(), H.PICTURE_ENTRY, "untouched")
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, flags=M.DECIDE_ONLY), inp))
        refused(lib, handoff(), H.PICTURE_ENTRY, "decisions only")
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp), inp))
        rect = Rect(0, 0, 128, 64)
        ok(lib, lib.svt_amd_encdec_picture_set_rect(world.ctx, world.pic, C.byref(rect)))
        refused(lib, handoff(), H.PICTURE_ENTRY, "rectangle")
        assert b"rectangle" in lib.svt_amd_last_error()
        ok(lib, lib.svt_amd_encdec_picture_set_rect(world.ctx, world.pic, None))
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        assert out.untouched()
        ok(lib, handoff())
        got = out.get()
        assert int(got["head"]["levels"]) > 0 and int(got["head"]["overflow"]) == 0 and int(got["head"]["bad_lcus"]) == 0 and int(got["head"]["bad_units"]) == 0
    finally:
        out.free()
        inp.free()
        world.free()


# ---- 6. two in flight ------------------------------------------------------------------------------------------------------------------------------------------------

def test_two_launches_in_flight_on_one_context(lib, oracle, gpu_ctx):
    """two pictures into two output sets back to back, one wait: both right - the launch has no working memory two launches could share"""
    names = ("b_motion_320x192_m5", "i_motion_416x240_m9")
    fx = [fixture(oracle, nm) for nm in names]
    recs = [Records(lib, gpu_ctx, f[0], f[1]) for f in fx]
    outs = [H.Outputs(lib, gpu_ctx, len(f[0]), *totals_of(f[2])) for f in fx]
    try:
        ok(lib, lib.svt_amd_synchronize(gpu_ctx))
        for r, o in zip(recs, outs):
            ok(lib, launch(lib, gpu_ctx, r, o))
        ok(lib, lib.svt_amd_synchronize(gpu_ctx))
        gots = [o.get() for o in outs]
        for nm, f, got in zip(names, fx, gots):
            clean_head(got["head"], totals_of(f[2]))
            compare(nm, f[2], got)
        assert gots[0]["levels"].tobytes() != gots[1]["levels"].tobytes()
    finally:
        for o in recs + outs:
            o.free()
