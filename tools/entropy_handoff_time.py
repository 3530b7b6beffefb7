#!/usr/bin/env python3
"""Measurement of the stream-ordered entropy hand-off (svt_amd_entropy_handoff_launch) beside the blocking caller of the same kernels (svt_amd_coeff_scan_picture), on the seeded
3840x2160 records of tests/test_gpu_coeffscan.py::random_records at coefficient densities 0.5 and 0.9, resident in HBM.
Per density, after two warm-up calls of each kind, 21 rounds that alternate the two entries in one process:
  launch    host time of the call (perf_counter around it, the lane idle before) and device time of its three kernels (svt_amd_timer_begin / _end around the call),
            exact-fit capacities;
  blocking  time from call to return on the same device arrays, worst-case capacities as its callers pass them, the bytes it downloads and the context scratch
            it asks for (from its carve: head, lcus and the two lists at the worst case; not measured).
Both entries run one chain of kernels; their lists are compared (byte for byte) before a number is printed, which holds the two host halves against each other.  Algorithmic bytes of the launch, from the shapes: the
coefficients of the coded blocks once, the record heads (1584 + 768 bytes an LCU), and the outputs (head, lcus, head copies, used lists); the share is of the
8 TB/s HBM peak, with the 6.3 TB/s copy rate of DESIGN 3.16 beside it.  Hand-off bytes: what a caller downloads per picture with the launch, against the full records.
Reported, not gated.  usage: entropy_handoff_time.py [output.txt]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import handofflib as H          # noqa: E402
import svtlib as S              # noqa: E402

W, HGT = 3840, 2160
ROUNDS, WARMUP = 21, 2
HBM_PEAK, COPY_RATE = 8.0e12, 6.3e12
vp, u32 = C.c_void_p, C.c_uint32


def coded_coefficient_bytes(works, results):
    """bytes of the s16 coefficients of every coded block: what one pass over the planes has to read"""
    total = 0
    for wk, rs in zip(works, results):
        n = int(wk["num_cus"])
        big = n == 1 and int(wk["cu"][0]["size"]) == 64
        for c in (range(1, 5) if big else range(n)):
            size = 32 if big else int(wk["cu"][c]["size"])
            for p in range(3):
                if rs["cu"][c]["cbf"][p]:
                    ts = size if p == 0 else (4 if size == 8 else size // 2)
                    total += 2 * ts * ts
    return total


def measure(lib, ctx, density, seed, lines):
    from test_gpu_coeffscan import random_records
    works, results = random_records(W, HGT, seed, density)
    n = len(works)
    ws, rs = works.dtype.itemsize, results.dtype.itemsize
    d_works, d_results = vp(), vp()
    for p, a in ((d_works, works), (d_results, results)):
        assert lib.svt_amd_device_alloc(ctx, a.nbytes, C.byref(p)) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_device_upload(ctx, p, a.ctypes.data, a.nbytes) == 0, lib.svt_amd_last_error()

    # the blocking entry once: totals for the exact-fit capacities, and the bytes to compare with
    b_lcus, b_groups, b_levels = np.zeros(n, S.COEFF_SCAN_LCU_DTYPE), np.zeros(H.MAX_GROUPS * n, S.COEFF_SCAN_GROUP_DTYPE), np.zeros(H.MAX_LEVELS * n, np.uint16)
    totals = (u32 * 2)()

    def blocking():
        t0 = time.perf_counter()
        rc = lib.svt_amd_coeff_scan_picture(ctx, d_works, ws, d_results, rs, 1, n, b_lcus.ctypes.data, b_groups.ctypes.data, len(b_groups), b_levels.ctypes.data,
                                            len(b_levels), C.byref(totals))
        dt = time.perf_counter() - t0
        assert rc == 0, lib.svt_amd_last_error()
        return dt
    blocking()
    ng, nl = int(totals[0]), int(totals[1])
    out = H.Outputs(lib, ctx, n, ng, nl)
    job = H.job(d_works.value, ws, d_results.value, rs, n, ng, nl)

    def launch():
        ms = C.c_float()
        assert lib.svt_amd_synchronize(ctx) == 0
        assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
        t0 = time.perf_counter()
        rc = lib.svt_amd_entropy_handoff_launch(ctx, C.byref(job), C.byref(out.out))
        dt = time.perf_counter() - t0
        assert rc == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
        return dt, ms.value * 1e-3
    for _ in range(WARMUP):
        launch()
        blocking()
    got = out.get()
    assert (int(got["head"]["groups"]), int(got["head"]["levels"]), int(got["head"]["overflow"])) == (ng, nl, 0)
    identical = got["lcus"].tobytes() == b_lcus.tobytes() and got["groups"].tobytes() == b_groups[:ng].tobytes() and got["levels"].tobytes() == b_levels[:nl].tobytes()
    host, dev, blk = [], [], []
    for _ in range(ROUNDS):
        h, d = launch()
        host.append(h), dev.append(d)
        blk.append(blocking())

    coeff = coded_coefficient_bytes(works, results)
    heads_in = n * (H.WORK_HEAD_BYTES + H.RESULT_HEAD_BYTES)
    outputs = 32 + n * H.LCU_BYTES + heads_in + 8 * ng + 2 * nl
    algorithmic = coeff + heads_in + outputs
    download = outputs
    blocking_download = 32 + n * H.LCU_BYTES + 8 * ng + 2 * nl
    blocking_scratch = 256 + H.round_up(n * H.LCU_BYTES) + n * (H.MAX_GROUPS * 8 + H.MAX_LEVELS * 2)
    full_records = n * (ws + rs)
    med = float(np.median(dev))
    lines += [
        "density %.1f (seed %d): %d LCUs, %d units, %d groups, %d levels; the two callers of the one chain return byte-identical lists: %s" % (
            density, seed, n, int(works["num_cus"].sum()), ng, nl, identical),
        "  launch    host time of the call   median %7.1f us  min %7.1f  max %7.1f" % (1e6 * float(np.median(host)), 1e6 * min(host), 1e6 * max(host)),
        "  launch    device time (3 kernels) median %7.1f us  min %7.1f  max %7.1f   (%d rounds after %d warm-ups)" % (1e6 * med, 1e6 * min(dev), 1e6 * max(dev), ROUNDS, WARMUP),
        "  launch    algorithmic bytes %.2f MB (coded coefficients once %.2f, heads in %.2f, outputs %.2f) -> %.2f TB/s = %.0f %% of the 8 TB/s HBM peak "
        "(%.0f %% of the 6.3 TB/s copy rate)" % (algorithmic / 1e6, coeff / 1e6, heads_in / 1e6, outputs / 1e6, algorithmic / med / 1e12, 100 * algorithmic / med / HBM_PEAK,
                                                100 * algorithmic / med / COPY_RATE),
        "  blocking  call to return          median %7.1f us  min %7.1f  max %7.1f   downloads %.2f MB (head, lcus, used lists), works in %.1f MB of context scratch" % (
            1e6 * float(np.median(blk)), 1e6 * min(blk), 1e6 * max(blk), blocking_download / 1e6, blocking_scratch / 1e6),
        "  hand-off  a caller downloads %.2f MB a picture (head 32 B, lcus %.2f, head copies %.2f, used lists %.2f) against %.1f MB of full 8-bit records (%.1f MB at 10 bit)"
        % (download / 1e6, n * H.LCU_BYTES / 1e6, heads_in / 1e6, (8 * ng + 2 * nl) / 1e6, full_records / 1e6,
           n * (S.LCU_WORK16_DTYPE.itemsize + S.LCU_RESULT16_DTYPE.itemsize) / 1e6)]
    out.free()
    for p in (d_works, d_results):
        lib.svt_amd_device_free(ctx, p)
    return identical


def main(argv):
    lib = H.declare(S.load_product())
    for f in (lib.svt_amd_timer_begin, lib.svt_amd_timer_end):
        f.restype = C.c_int
    lib.svt_amd_timer_begin.argtypes, lib.svt_amd_timer_end.argtypes = [vp], [vp, C.POINTER(C.c_float)]
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, HGT, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    lines = ["# svt_amd_entropy_handoff_launch beside svt_amd_coeff_scan_picture, one %dx%d picture of seeded records resident in HBM, entries alternating in one process, "
             "one run on one MI355X" % (W, HGT)]
    same = [measure(lib, ctx, density, seed, lines) for density, seed in ((0.5, 21), (0.9, 22))]
    lib.svt_amd_context_destroy(ctx)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if argv:
        with open(argv[0], "w") as f:
            f.write(text)
    assert all(same)


if __name__ == "__main__":
    main(sys.argv[1:])
