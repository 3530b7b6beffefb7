"""Entropy hand-off pre-scan on the device (svt-hevc_amd/csrc/handoff_kernels.hip) through the C-ABI: the blocking svt_amd_coeff_scan_picture against
the CPU checker (pinned on the reference's coder by tests/test_oracle_coeffscan.py) - block records, sub-block groups and levels bit for bit - on the
recorded encodes, on a seeded 4K picture from device arrays, and, where oracle/_ref travels with the snapshot, straight against the reference's coder.  Then
what is the blocking entry's own around the kernels it shares with the stream-ordered launch (tests/test_gpu_entropy_handoff.py): host against device arrays,
capacities that do not fit, malformed records, more LCUs than a launch takes."""
import ctypes as C

import numpy as np
import pytest

import handoff_numpy as N
import handofflib as H
import svtlib as S
import test_gpu_entropy_handoff as E
from pa_batch_util import is_sentinel, make_context, refused
from test_oracle_encodepass_golden import ALL, is16, load_case

pytestmark = pytest.mark.gpu
vp, u32 = C.c_void_p, C.c_uint32
CASES = [c for c in ALL if not c.startswith(("dlf_", "sao_"))]


def sig(lib):
    lib.svt_amd_coeff_scan_picture.restype = C.c_int
    lib.svt_amd_coeff_scan_picture.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp, vp, u32, vp, u32, C.POINTER(u32 * 2)]


def device_scan(lib, ctx, works, wstride, results, rstride, device, n, gcap=None, lcap=None):
    gcap, lcap = gcap if gcap is not None else 384 * n, lcap if lcap is not None else 6144 * n
    lcus, groups, levels = np.zeros(n, S.COEFF_SCAN_LCU_DTYPE), np.zeros(max(gcap, 1), S.COEFF_SCAN_GROUP_DTYPE), np.zeros(max(lcap, 1), np.uint16)
    totals = (u32 * 2)()
    rc = lib.svt_amd_coeff_scan_picture(ctx, works, wstride, results, rstride, device, n, lcus.ctypes.data, groups.ctypes.data, gcap, levels.ctypes.data, lcap,
                                        C.byref(totals))
    return rc, lcus, groups, levels, (int(totals[0]), int(totals[1]))


def oracle_scan(oracle, work, res):
    oracle.svt_oracle_coeff_scan_lcu.restype, oracle.svt_oracle_coeff_scan_lcu.argtypes = C.c_int, [vp, vp, vp, vp, vp]
    lcu = np.zeros(1, S.COEFF_SCAN_LCU_DTYPE)
    groups, levels = np.zeros(384, S.COEFF_SCAN_GROUP_DTYPE), np.zeros(6144, np.uint16)
    oracle.svt_oracle_coeff_scan_lcu(work.ctypes.data, res.ctypes.data, lcu.ctypes.data, groups.ctypes.data, levels.ctypes.data)
    return lcu[0], groups, levels


def compare_lcu(tag, want, wg, wl, got, groups, levels):
    assert int(got["groups"]) == int(want["groups"]) and int(got["levels"]) == int(want["levels"]), (tag, got["groups"], want["groups"], got["levels"], want["levels"])
    assert np.array_equal(got["tu"], want["tu"]), (tag, np.argwhere(got["tu"] != want["tu"])[:4].tolist())
    gb, lb, ng, nl = int(got["group_base"]), int(got["level_base"]), int(got["groups"]), int(got["levels"])
    assert np.array_equal(groups[gb:gb + ng], wg[:ng]), (tag, "groups")
    assert np.array_equal(levels[lb:lb + nl], wl[:nl]), (tag, "levels")


@pytest.mark.parametrize("name", CASES)
def test_prescan_of_recorded_pictures_matches_the_checker(product, oracle, gpu_ctx, name):
    lib = product
    sig(lib)
    g, w, h = load_case(name)
    works, results = np.ascontiguousarray(g["work"]), np.ascontiguousarray(g["result"])
    n = len(works)
    rc, lcus, groups, levels, totals = device_scan(lib, gpu_ctx, works.ctypes.data, works.dtype.itemsize, results.ctypes.data, results.dtype.itemsize, 0, n)
    assert rc == 0, lib.svt_amd_last_error()
    gsum = lsum = 0
    for k in range(n):
        want, wg, wl = oracle_scan(oracle, works[k:k + 1], results[k:k + 1])
        assert int(lcus[k]["group_base"]) == gsum and int(lcus[k]["level_base"]) == lsum, (name, k)
        compare_lcu((name, k), want, wg, wl, lcus[k], groups, levels)
        gsum, lsum = gsum + int(want["groups"]), lsum + int(want["levels"])
    assert totals == (gsum, lsum) and lsum > 0


def random_records(w, h, seed, density):
    """unit trees of tools/encodepass_bench.py with random coefficient planes: cbf / count records consistent with the planes"""
    import sys, os
    sys.path.insert(0, os.path.join(S.ROOT, "tools"))
    import encodepass_bench as EPB
    rng = np.random.default_rng(seed)
    works = EPB.works_of(w, h, 30, seed, None, 0.5)
    n = len(works)
    results = np.zeros(n, S.LCU_RESULT_DTYPE)
    yy, xx = np.mgrid[:64, :64]
    for k in range(n):
        wk, rs = works[k], results[k]
        for c in range(int(wk["num_cus"])):
            cu = wk["cu"][c]
            x, y, s = int(cu["x"]), int(cu["y"]), int(cu["size"])
            for p in range(3):
                ts = s if p == 0 else (4 if s == 8 else s // 2)
                if rng.random() < 0.25:
                    continue                                        # cbf 0: whatever the plane holds there is not coded
                kind = rng.random()
                if kind < 0.2:
                    blk = np.zeros((ts, ts), np.int16)
                    blk[0, 0] = rng.choice([-2, 1, 4])
                else:
                    fy, fx = np.mgrid[:ts, :ts]
                    blk = (rng.integers(-60, 61, (ts, ts)) * (rng.random((ts, ts)) < density) / (1 + (fx + fy) ** 1.3)).astype(np.int16)
                if not blk.any():
                    continue
                plane = rs["coeff_y"].reshape(64, 64) if p == 0 else rs[("coeff_cb", "coeff_cr")[p - 1]].reshape(32, 32)
                ox, oy = (x, y) if p == 0 else (x // 2, y // 2)
                plane[oy:oy + ts, ox:ox + ts] = blk
                rs["cu"][c]["cbf"][p], rs["cu"][c]["nz"][p] = 1, int((blk != 0).sum())
    return works, results


@pytest.mark.parametrize("w,h,seed,density", [(3840, 2160, 21, 0.5), (1920, 1080, 22, 0.9)])
def test_prescan_of_a_seeded_picture_from_device_arrays(product, oracle, w, h, seed, density):
    """BASELINE configs[2] / [1] picture sizes: records resident in HBM (what svt_amd_encode_picture_device leaves); every 7th LCU against the checker,
    all of them through what does not depend on it: the lists are packed in LCU order and hold exactly the non-zero coefficients of the coded blocks"""
    import torch
    lib = product
    sig(lib)
    ctx = vp()
    assert lib.svt_amd_context_create(0, w, h, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    try:
        works, results = random_records(w, h, seed, density)
        n = len(works)
        dw, dr = torch.from_numpy(works.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(results.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        rc, lcus, groups, levels, totals = device_scan(lib, ctx, dw.data_ptr(), works.dtype.itemsize, dr.data_ptr(), results.dtype.itemsize, 1, n)
        assert rc == 0, lib.svt_amd_last_error()
        assert np.array_equal(lcus["group_base"], np.concatenate([[0], np.cumsum(lcus["groups"].astype(np.int64))[:-1]]))
        assert np.array_equal(lcus["level_base"], np.concatenate([[0], np.cumsum(lcus["levels"].astype(np.int64))[:-1]]))
        assert totals == (int(lcus["groups"].sum()), int(lcus["levels"].sum()))
        coded = int(sum(int(results[k]["cu"]["nz"][:int(works[k]["num_cus"])][results[k]["cu"]["cbf"][:int(works[k]["num_cus"])] != 0].sum()) for k in range(n)))
        assert totals[1] == coded and (levels[:totals[1]] != 0).all()
        for k in range(0, n, 7):
            want, wg, wl = oracle_scan(oracle, works[k:k + 1], results[k:k + 1])
            compare_lcu((w, h, k), want, wg, wl, lcus[k], groups, levels)
        # the capacities are checked, not trusted
        rc, _, _, _, need = device_scan(lib, ctx, dw.data_ptr(), works.dtype.itemsize, dr.data_ptr(), results.dtype.itemsize, 1, n, gcap=totals[0] - 1, lcap=totals[1])
        assert rc != 0 and need == totals
    finally:
        lib.svt_amd_context_destroy(ctx)


def test_device_records_code_the_reference_bytes(product, gpu_ctx):
    """no checker in between: the device's records through the CABAC loop of integration/svt_coeff_scan_consumer.h, the recorded coefficients through the
    reference's EncodeQuantizedCoefficients_generic, on two states of the reference's arithmetic coder (needs oracle/_ref on the box)"""
    ref = S.load_ref()
    if ref is None or not hasattr(ref, "svt_ref_cabac_new"):
        pytest.skip("oracle/_ref/libsvtref.so is not on this box")
    from test_oracle_coeffscan import state_of
    ref.svt_ref_cabac_new.restype, ref.svt_ref_cabac_new.argtypes = vp, [u32]
    ref.svt_ref_cabac_free.restype, ref.svt_ref_cabac_free.argtypes = None, [vp]
    ref.svt_ref_cabac_code_raw.restype, ref.svt_ref_cabac_code_raw.argtypes = None, [vp, u32, u32, u32, vp, u32, u32, u32, C.c_int]
    ref.svt_ref_cabac_code_scan.restype, ref.svt_ref_cabac_code_scan.argtypes = None, [vp, u32, u32, vp, vp, vp]
    ref.svt_ref_cabac_state.restype, ref.svt_ref_cabac_state.argtypes = u32, [vp, vp, u32]
    lib = product
    sig(lib)
    for name in ("b_motion_320x192_m5", "i_motion_416x240_m9", "p10_motion_320x192_m7"):
        g, w, h = load_case(name)
        works, results = np.ascontiguousarray(g["work"]), np.ascontiguousarray(g["result"])
        n = len(works)
        rc, lcus, groups, levels, totals = device_scan(lib, gpu_ctx, works.ctypes.data, works.dtype.itemsize, results.ctypes.data, results.dtype.itemsize, 0, n)
        assert rc == 0, lib.svt_amd_last_error()
        a, b = ref.svt_ref_cabac_new(7), ref.svt_ref_cabac_new(7)
        try:
            blocks = 0
            for k in range(n):
                wk, rs = works[k], results[k]
                ncu = int(wk["num_cus"])
                big = ncu == 1 and int(wk["cu"][0]["size"]) == 64
                gl = np.ascontiguousarray(groups[int(lcus[k]["group_base"]):int(lcus[k]["group_base"]) + 384])
                ll = np.ascontiguousarray(levels[int(lcus[k]["level_base"]):int(lcus[k]["level_base"]) + 6144])
                for c in (range(1, 5) if big else range(ncu)):
                    cu = wk["cu"][0 if big else c]
                    size = 32 if big else int(cu["size"])
                    x, y = (32 * ((c - 1) & 1), 32 * ((c - 1) >> 1)) if big else (int(cu["x"]), int(cu["y"]))
                    for p in range(3):
                        if not rs["cu"][c]["cbf"][p]:
                            continue
                        ts = size if p == 0 else (4 if size == 8 else size // 2)
                        plane = rs["coeff_y"].reshape(64, 64) if p == 0 else rs[("coeff_cb", "coeff_cr")[p - 1]].reshape(32, 32)
                        st = 64 if p == 0 else 32
                        full = np.zeros((32, st), np.int16)
                        full[:ts, :ts] = plane[(y >> (p > 0)):, (x >> (p > 0)):][:ts, :ts]
                        ref.svt_ref_cabac_code_raw(a, ts, int(cu["pred_mode"]), int(cu["intra_luma_mode"]), full.ctypes.data, st, p, int(rs["cu"][c]["nz"][p]), 0)
                        tu = np.ascontiguousarray(lcus[k]["tu"][p][c:c + 1])
                        ref.svt_ref_cabac_code_scan(b, ts, p, tu.ctypes.data, gl.ctypes.data, ll.ctypes.data)
                        blocks += 1
            sa, sb = state_of(ref, a), state_of(ref, b)
            assert blocks > 20 and np.array_equal(sa, sb), (name, blocks)
        finally:
            ref.svt_ref_cabac_free(a), ref.svt_ref_cabac_free(b)


# ---- what is the blocking entry's own: the kernels are the launch's (tests/test_gpu_entropy_handoff.py) ------------------------------------------------------

def host_bytes(a, stride, at=1):
    """the records of `a` as a byte array in which they lie `stride` bytes apart from the odd offset `at` on: (keep-alive, address)"""
    rows = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    buf = np.zeros(at + len(a) * stride, np.uint8)
    buf[at:].reshape(len(a), stride)[:, :rows.shape[1]] = rows
    return buf, buf.ctypes.data + at


def lists_untouched(got, groups=0, levels=0):
    """nothing at or behind `groups` / `levels` elements of the host lists was written"""
    return is_sentinel(got["groups"][groups:]) and is_sentinel(got["levels"][levels:])


@pytest.mark.parametrize("name", ["i_noise_200x136_m6", "sao_p_noise_320x256_m8"])
def test_host_and_device_arrays_give_the_same_bytes(product, oracle, gpu_ctx, name):
    """the same records as device arrays and as host arrays - these at an odd address and an odd stride, which only an upload can take - at the worst-case capacities
    and at the exact fit: the checker's lists, the same bytes either way, nothing at or behind the totals written"""
    lib = H.declare(product)
    works, results, exp = E.fixture(oracle, name)
    n, totals = len(works), E.totals_of(exp)
    assert (name, n) == ("i_noise_200x136_m6", 12) or (name, totals) == ("sao_p_noise_320x256_m8", (16001, 159356))
    recs = E.Records(lib, gpu_ctx, works, results)
    ws, rs = works.dtype.itemsize + 3, results.dtype.itemsize + 1
    keep_w, h_works = host_bytes(works, ws)
    keep_r, h_results = host_bytes(results, rs)
    try:
        for gcap, lcap in ((H.MAX_GROUPS * n, H.MAX_LEVELS * n), totals):
            rc, dev = H.scan_picture(lib, gpu_ctx, recs.d_works, recs.work_stride, recs.d_results, recs.result_stride, 1, n, gcap, lcap)
            assert rc == 0, lib.svt_amd_last_error()
            rc, host = H.scan_picture(lib, gpu_ctx, h_works, ws, h_results, rs, 0, n, gcap, lcap)
            assert rc == 0, lib.svt_amd_last_error()
            for got in (dev, host):
                assert got["totals"] == totals, (name, gcap)
                E.compare((name, gcap), exp, got)
                assert lists_untouched(got, *totals), (name, gcap)
            assert dev["lcus"].tobytes() == host["lcus"].tobytes() and dev["groups"].tobytes() == host["groups"].tobytes(), (name, gcap)
            assert dev["levels"].tobytes() == host["levels"].tobytes(), (name, gcap)
    finally:
        recs.free()
    del keep_w, keep_r


def test_capacities_that_do_not_fit_are_refused_with_the_need(product, oracle, gpu_ctx):
    """groups one short, levels one short, both 0, from device and from host arrays: SVT_AMD_ERR_RESOURCES, totals what the picture needs, lcus[] the fitting
    run's, neither host list touched"""
    lib = H.declare(product)
    name = "sao_p_noise_320x256_m8"
    works, results, exp = E.fixture(oracle, name)
    n, totals = len(works), E.totals_of(exp)
    assert totals == (16001, 159356)
    recs = E.Records(lib, gpu_ctx, works, results)
    arrays = ((recs.d_works, recs.work_stride, recs.d_results, recs.result_stride, 1), (works.ctypes.data, works.dtype.itemsize, results.ctypes.data, results.dtype.itemsize, 0))
    try:
        rc, fit = H.scan_picture(lib, gpu_ctx, *arrays[0], n, *totals)
        assert rc == 0, lib.svt_amd_last_error()
        E.compare(name, exp, fit)
        for gcap, lcap in ((totals[0] - 1, totals[1]), (totals[0], totals[1] - 1), (0, 0)):
            for a in arrays:
                rc, got = H.scan_picture(lib, gpu_ctx, *a, n, gcap, lcap)
                assert rc == H.ERR_RESOURCES, (gcap, lcap, rc, lib.svt_amd_last_error())
                assert lib.svt_amd_last_error() == b"svt_amd_coeff_scan_picture: %d groups / %d levels do not fit the capacities %d / %d" % (totals + (gcap, lcap))
                assert got["totals"] == totals and got["lcus"].tobytes() == fit["lcus"].tobytes(), (gcap, lcap)
                assert lists_untouched(got), (gcap, lcap)
    finally:
        recs.free()


def test_malformed_records_are_refused_and_the_context_goes_on(product, oracle, gpu_ctx):
    """the seven rewritten records of the launch's test (handoff_numpy.malformed; the launch runs them safely), as device arrays with 128 KB of the test's own memory
    around each and as host arrays - these at capacities of 0, since malformed records are judged before the capacities: SVT_AMD_ERR_BAD_PARAM with both counts and
    both first LCUs in the text, totals and lcus[] what the checker gives on records in which the refused slots are not coded, neither host list touched; then the
    good records on the same context"""
    lib = H.declare(product)
    name = "sao_p_noise_320x256_m8"
    good_w, good_r, exp_good = E.fixture(oracle, name)
    works, results, rewritten = N.malformed(good_w, good_r)
    n = len(works)
    exp = E.expected_of(oracle, *N.sanitized(works, results))
    totals = E.totals_of(exp)
    recs = E.Records(lib, gpu_ctx, works, results, margin=E.MARGIN)
    try:
        for a, gcap, lcap in (((recs.d_works, recs.work_stride, recs.d_results, recs.result_stride, 1), H.MAX_GROUPS * n, H.MAX_LEVELS * n),
                              ((works.ctypes.data, works.dtype.itemsize, results.ctypes.data, results.dtype.itemsize, 0), 0, 0)):
            rc, got = H.scan_picture(lib, gpu_ctx, *a, n, gcap, lcap)
            refused(lib, rc, H.BLOCKING_ENTRY, a[4])
            assert b"2 bad LCUs (first 2), 5 bad units (first in LCU 7)" in lib.svt_amd_last_error(), lib.svt_amd_last_error()
            assert got["totals"] == totals, a[4]
            E.compare(name, exp, got, lists=(False, False))
            for k in rewritten:
                assert (got["lcus"][k]["tu"][:, N.bad_slots(works[k])] == E.NOTHING).all(), k
            assert lists_untouched(got), a[4]
        good_totals = E.totals_of(exp_good)
        rc, got = H.scan_picture(lib, gpu_ctx, good_w.ctypes.data, good_w.dtype.itemsize, good_r.ctypes.data, good_r.dtype.itemsize, 0, n, *good_totals)
        assert rc == 0, lib.svt_amd_last_error()
        assert got["totals"] == good_totals and lists_untouched(got, *good_totals)
        E.compare(name, exp_good, got)
    finally:
        recs.free()


@pytest.mark.parametrize("n", [1025, H.MAX_LCUS + 1])
def test_more_lcus_than_a_launch_takes(product, oracle, n):
    """the 12 records of one picture repeated as host arrays at the smallest strides, at the exact fit, in a context of its own (its scratch grows with the picture):
    bases = exclusive sums of the checker's counts, the totals, the lists of the first, the last and every 997th LCU; the launch entry still refuses 16385 LCUs"""
    lib = H.declare(product)
    works, results, exp12 = E.fixture(oracle, "i_noise_200x136_m6")
    assert len(works) == 12
    idx = np.arange(n) % 12
    exp = [exp12[k] for k in idx]
    totals = E.totals_of(exp)
    wb = np.ascontiguousarray(works.view(np.uint8).reshape(12, -1)[:, :H.WORK_HEAD_BYTES][idx])
    rb = np.ascontiguousarray(results.view(np.uint8).reshape(12, -1)[:, :H.RESULT_MIN_BYTES][idx])
    if n > H.MAX_LCUS:                          # refused on the host, before the job's arrays or the outputs are read: host memory stands for them
        out = H.Out()
        out.head, out.lcus, out.groups, out.levels = (wb.ctypes.data + 64 * i for i in range(4))
        job = H.job(wb.ctypes.data, H.WORK_HEAD_BYTES, rb.ctypes.data, H.RESULT_MIN_BYTES, n, *totals)
    ctx = make_context(lib, 640, 384, 1)
    try:
        if n > H.MAX_LCUS:
            refused(lib, lib.svt_amd_entropy_handoff_launch(ctx, C.byref(job), C.byref(out)), H.ENTRY, n)
        rc, got = H.scan_picture(lib, ctx, wb.ctypes.data, H.WORK_HEAD_BYTES, rb.ctypes.data, H.RESULT_MIN_BYTES, 0, n, *totals)
        assert rc == 0, lib.svt_amd_last_error()
        assert got["totals"] == totals and lists_untouched(got, *totals), n
        E.compare(n, exp, got, sorted(set(range(0, n, 997)) | {0, n - 1}))
    finally:
        lib.svt_amd_context_destroy(ctx)
