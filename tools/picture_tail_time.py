#!/usr/bin/env python3
"""Two measurements of the picture tail on the device (svt_amd_encdec_picture_tail_launch) on one 3840x2160 picture of seeded records (2,040 LCUs, all-intra quadtrees
of 8 to 32 with a QP per unit, encoded once by svt_amd_encode_picture), one device, profiler off, two warm-up calls.
(a) device time: svt_amd_timer_begin / _end around ONE tail on the context's lane, median of seven, for the full tail and for the stage sets that isolate its parts
    (SVT_AMD_TAIL_REFERENCE alone is k_tail_pad alone), with the bytes each moves and what those bytes cost at the device's HBM bandwidth.  The new kernels one by
    one come from a kernel trace of this script (a run of its own).  Neither figure is gated.
(b) call time: wall time from the call to completed results of the parent's three blocking calls (svt_amd_encdec_picture_deblock, _sao, _reference: host records in,
    parameters out) and of the tail plus one svt_amd_synchronize (records and results stay in HBM), on two picture objects that hold the same encoded picture,
    alternated, five each.  Reported: both series, the difference of the medians and the condition - the tail's median does not exceed the blocking median by more than
    the spread of the blocking series.
The outputs of both paths are compared byte for byte in the same run (padded planes and parameters) before any number is printed.
usage: picture_tail_time.py [output.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlib as S              # noqa: E402
import tail_numpy as N          # noqa: E402
import taillib as T             # noqa: E402
from test_oracle_saodec_golden import LCU, params_of   # noqa: E402
from test_oracle_encodepass_golden import load_case     # noqa: E402

W, H = 3840, 2160
HBM_GBS = 6300.0                # what a float4 copy reaches on an MI355X (8 TB/s peak), GB/s
vp = C.c_void_p
D, SD, A, R = N.DEBLOCK, N.SAO_DECIDE, N.SAO_APPLY, N.REFERENCE


def seeded_works(w, h, seed):
    """all-intra quadtrees of 8 to 32 over every LCU, a QP per unit, smooth seeded source samples"""
    rng = np.random.default_rng(seed)
    wl, hl = (w + 63) // 64, (h + 63) // 64
    works = np.zeros(wl * hl, S.LCU_WORK_DTYPE)
    yy, xx = np.mgrid[0:h, 0:w]
    luma = (128 + 60 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + rng.integers(-12, 13, (h, w))).clip(0, 255).astype(np.uint8)
    chroma = [(128 + 30 * np.sin(xx[::2, ::2] / (41.0 + 9 * k))).astype(np.uint8) for k in range(2)]
    for n in range(wl * hl):
        ox, oy = 64 * (n % wl), 64 * (n // wl)
        lw, lh = min(64, w - ox), min(64, h - oy)
        units = []

        def rec(x, y, s):
            if x >= lw or y >= lh:
                return
            if s > 32 or x + s > lw or y + s > lh or (s > 8 and rng.random() < 0.45):
                for dy, dx in ((0, 0), (0, s // 2), (s // 2, 0), (s // 2, s // 2)):
                    rec(x + dx, y + dy, s // 2)
            else:
                units.append((x, y, s))
        rec(0, 0, 64)
        k = len(units)
        wk = works[n]
        wk["lcu_x"], wk["lcu_y"], wk["num_cus"], wk["slice_type"] = ox, oy, k, 2
        wk["tile_left"], wk["tile_top"], wk["tile_right"] = ox == 0, oy == 0, ox + 64 >= w
        cu = wk["cu"]
        cu["x"][:k], cu["y"][:k], cu["size"][:k] = zip(*units)
        cu["pred_mode"][:k] = 2
        cu["intra_luma_mode"][:k] = rng.integers(0, 35, k)
        cu["qp"][:k] = rng.integers(24, 40, k)
        cu["chroma_qp"][:k] = cu["qp"][:k]
        sy = np.zeros((64, 64), np.uint8)
        sy[:lh, :lw] = luma[oy:oy + lh, ox:ox + lw]
        wk["src_y"] = sy.reshape(-1)
        for nm, pl in zip(("src_cb", "src_cr"), chroma):
            sc = np.zeros((32, 32), np.uint8)
            sc[:lh // 2, :lw // 2] = pl[oy // 2:(oy + lh) // 2, ox // 2:(ox + lw) // 2]
            wk[nm] = sc.reshape(-1)
    return works


def main(argv):
    from test_gpu_encodepass import DeblockParams
    lib = T.declare(S.load_product())
    lib.svt_amd_encdec_picture_create.restype, lib.svt_amd_encdec_picture_create.argtypes = C.c_int, [vp, C.c_uint16, C.c_uint16, C.c_int, C.POINTER(vp)]
    lib.svt_amd_encode_picture.restype, lib.svt_amd_encode_picture.argtypes = C.c_int, [vp] * 4
    lib.svt_amd_encdec_picture_deblock.restype, lib.svt_amd_encdec_picture_deblock.argtypes = C.c_int, [vp, vp, vp, vp, C.POINTER(DeblockParams), vp, vp, vp]
    lib.svt_amd_encdec_picture_sao.restype, lib.svt_amd_encdec_picture_sao.argtypes = C.c_int, [vp] * 9
    lib.svt_amd_encdec_picture_reference.restype = C.c_int
    lib.svt_amd_encdec_picture_reference.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_destroy.argtypes = [vp, vp]

    def ok(rc):
        assert rc == 0, lib.svt_amd_last_error()
    ctx = vp()
    ok(lib.svt_amd_context_create(0, W, H, 1, C.byref(ctx)))
    nl = S.lcu_count(W, H)
    works = seeded_works(W, H, 27)
    P = params_of(load_case("sao_i_noise_200x136_m6")[0]["sao"][0])      # the rate inputs of a recorded I picture
    pics, results = [vp(), vp()], []
    for pic in pics:                    # [0] the blocking calls' object, [1] the tail's: the same encoded picture in both
        ok(lib.svt_amd_encdec_picture_create(ctx, W, H, 1, C.byref(pic)))
        res = np.zeros(nl, S.LCU_RESULT_DTYPE)
        ok(lib.svt_amd_encode_picture(ctx, pic, works.ctypes.data, res.ctypes.data))
        results.append(res)
    d_works, d_results, d_par, d_chk = vp(), vp(), vp(), vp()
    for p, b in ((d_works, works.nbytes), (d_results, results[1].nbytes), (d_par, nl * 72), (d_chk, 256)):
        ok(lib.svt_amd_device_alloc(ctx, b, C.byref(p)))
    ok(lib.svt_amd_device_upload(ctx, d_works, works.ctypes.data, works.nbytes))
    ok(lib.svt_amd_device_upload(ctx, d_results, results[1].ctypes.data, results[1].nbytes))
    ok(lib.svt_amd_encdec_picture_tail_warmup(ctx, pics[1], 80, 80))
    ref_t, ref_b = S.RefPicture(), S.RefPicture()

    def job(stages):
        return T.job(d_works.value, works.dtype.itemsize, d_results.value, results[1].dtype.itemsize, stages, 2, (0, 0), P, None, (80, 80))
    prm = DeblockParams()
    prm.slice_type = 2
    dec_b = np.zeros(nl, LCU)

    def blocking():
        t0 = time.perf_counter()
        ok(lib.svt_amd_encdec_picture_deblock(ctx, pics[0], works.ctypes.data, results[0].ctypes.data, C.byref(prm), None, None, None))
        ok(lib.svt_amd_encdec_picture_sao(ctx, pics[0], works.ctypes.data, P.ctypes.data, None, dec_b.ctypes.data, None, None, None))
        ok(lib.svt_amd_encdec_picture_reference(ctx, pics[0], 80, 80, C.byref(ref_b), None, None, None))
        return (time.perf_counter() - t0) * 1e3
    full = job(D | SD | A | R)

    def tail():
        t0 = time.perf_counter()
        ok(lib.svt_amd_encdec_picture_tail_launch(ctx, pics[1], C.byref(full), d_par, d_chk, C.byref(ref_t)))
        ok(lib.svt_amd_synchronize(ctx))
        return (time.perf_counter() - t0) * 1e3

    # ---- the outputs first: a number is never reported for wrong results ----
    blocking(), tail()
    sizes = [(H + 160) * (W + 160), (H // 2 + 80) * (W // 2 + 80), (H // 2 + 80) * (W // 2 + 80)]
    identical = True
    for rb, rt, n in zip((ref_b.d_y, ref_b.d_cb, ref_b.d_cr), (ref_t.d_y, ref_t.d_cb, ref_t.d_cr), sizes):
        a, b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        ok(lib.svt_amd_device_download(ctx, a.ctypes.data, vp(rb), n)), ok(lib.svt_amd_device_download(ctx, b.ctypes.data, vp(rt), n))
        identical = identical and a.tobytes() == b.tobytes()
    dec_t, chk = np.zeros(nl, LCU), np.zeros(1, N.CHECK_DTYPE)
    ok(lib.svt_amd_device_download(ctx, dec_t.ctypes.data, d_par, dec_t.nbytes)), ok(lib.svt_amd_device_download(ctx, chk.ctypes.data, d_chk, 16))
    identical = identical and dec_t.tobytes() == dec_b.tobytes() and chk[0].tolist() == (0, N.NONE, 0, N.NONE)
    assert identical, "the tail and the blocking calls differ"

    # ---- (b) call time, alternated (one warm-up of each is behind us; one more) ----
    blocking(), tail()
    tb, tt = [], []
    for rep in range(5):
        tb.append(blocking()), tt.append(tail())

    # ---- (a) device time ----
    plane, padded = W * H * 3 // 2, sum(sizes)
    rec_bytes = nl * (T.LIST_BYTES + T.RESULT_CU_BYTES)
    maps_out = (W // 8) * (H // 8) * 13 + (W // 4) * (H // 4) + nl * (4 + 72)
    moved = {"reference (k_tail_pad alone)": plane + padded,
             "deblock (k_tail_maps, k_tail_check, strengths, copy, deblocking)": rec_bytes + 2 * plane + maps_out + 2 * plane + 2 * plane,
             "deblock + decide (adds k_tail_composite, statistics, decision)": None, "full tail": None}
    sets = {"reference (k_tail_pad alone)": R, "deblock (k_tail_maps, k_tail_check, strengths, copy, deblocking)": D,
            "deblock + decide (adds k_tail_composite, statistics, decision)": D | SD, "full tail": D | SD | A | R}
    moved["deblock + decide (adds k_tail_composite, statistics, decision)"] = moved["deblock (k_tail_maps, k_tail_check, strengths, copy, deblocking)"] + 3 * plane + 2 * plane
    moved["full tail"] = moved["deblock + decide (adds k_tail_composite, statistics, decision)"] + 2 * plane + plane + padded
    device = {}
    for name, stages in sets.items():
        j, times = job(stages), []
        for k in range(9):
            ms = C.c_float()
            ok(lib.svt_amd_timer_begin(ctx))
            ok(lib.svt_amd_encdec_picture_tail_launch(ctx, pics[1], C.byref(j), d_par, d_chk, C.byref(ref_t)))
            ok(lib.svt_amd_timer_end(ctx, C.byref(ms)))
            if k >= 2:
                times.append(ms.value * 1e3)
        device[name] = {"us_median": round(float(np.median(times)), 1), "us_min": round(min(times), 1), "us_max": round(max(times), 1), "series_us": [round(v, 1) for v in times],
                        "bytes_moved_estimate": moved[name], "us_at_hbm_copy_rate": round(moved[name] / HBM_GBS / 1e3, 1)}

    def series(t):
        return {"ms_median": round(float(np.median(t)), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "series_ms": [round(v, 3) for v in t]}
    diff, spread = float(np.median(tt)) - float(np.median(tb)), max(tb) - min(tb)
    out = {"width": W, "height": H, "lcus": nl, "units": int(works["num_cus"].sum()), "sao_lcus_on": int((dec_b["type"] != 0).any(axis=1).sum()),
           "outputs_byte_identical": bool(identical), "hbm_copy_rate_gbs": HBM_GBS, "device_time": device,
           "call_time": {"blocking_three_calls": series(tb), "tail_plus_one_synchronize": series(tt), "median_difference_ms": round(diff, 3),
                         "blocking_spread_ms": round(spread, 3), "condition_tail_no_slower_than_blocking_by_more_than_its_spread": bool(diff <= spread),
                         "host_bytes_the_blocking_calls_upload": int(works.nbytes + (W // 8) * (H // 8) * 13 + (W // 4) * (H // 4) + nl * (2 + 72))}}
    line = json.dumps(out)
    print(line)
    if argv:
        with open(argv[0], "w") as f:
            f.write(line + "\n")
    for p in (d_works, d_results, d_par, d_chk):
        lib.svt_amd_device_free(ctx, p)
    for pic in pics:
        lib.svt_amd_encdec_picture_destroy(ctx, pic)
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main(sys.argv[1:])
