#!/usr/bin/env python3
"""The side statistics of a 64-picture 4K batch in their two forms:
  blocking  the three single-picture entries per picture (svt_amd_picture_stats, svt_amd_picture_ac_energy, svt_amd_zz_sad_picture): 192 calls, each
            ending in a wait for the device
  batch     ONE svt_amd_side_stats_batch_launch and one download per kind
usage: side_stats_profile.py blocking|batch|wall [pictures]
`blocking` and `batch` run the form twice (the first pass loads the code objects) - run them under `rocprofv3 --kernel-trace --stats -- python ...`
for the kernel table (profiles/summarize_rocpd.py); `blocking` also works with a library that has no batched form (SVT_PRODUCT_LIB).  `wall` times
both forms on the host, five passes each, alternated, and prints the medians as one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sidelib as L      # noqa: E402
import svtlib as S       # noqa: E402

W, H = 3840, 2160
vp = C.c_void_p


def main():
    form = sys.argv[1] if len(sys.argv) > 1 else "wall"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    lib = S.load_product()
    lib.svt_amd_picture_stats.restype, lib.svt_amd_picture_stats.argtypes = C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.svt_amd_picture_ac_energy.restype, lib.svt_amd_picture_ac_energy.argtypes = C.c_int, [vp, C.c_int, vp]
    lib.svt_amd_zz_sad_picture.restype, lib.svt_amd_zz_sad_picture.argtypes = C.c_int, [vp, C.c_int, C.c_int, vp]
    if form != "blocking":
        L.declare(lib)
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, n, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    base = [S.gen_luma(("objects", "motion", "noise", "static")[i], W, H, 1, 5 + i) for i in range(4)]
    for i in range(n):
        f = np.ascontiguousarray(np.roll(base[i % 4], (3 * (i // 4), 5 * (i // 4)), (0, 1)))
        assert lib.svt_amd_picture_upload(ctx, i, f.ctypes.data, W, W, H) == 0, lib.svt_amd_last_error()
    nl = S.lcu_count(W, H)
    stats = np.zeros((n, nl), S.PA_LCU_STATS_DTYPE)
    hist, ravg, total = np.zeros((n, 4, 4, 256), np.uint32), np.zeros((n, 16), np.uint8), np.zeros(n, np.uint64)
    energy, zz = np.zeros((n, nl, 5), np.uint64), np.zeros((n, nl), L.ZZ_DTYPE)

    def blocking():
        for i in range(n):
            assert lib.svt_amd_picture_stats(ctx, i, stats[i].ctypes.data, 4, 4, hist[i].ctypes.data, ravg[i].ctypes.data, total[i:].ctypes.data) == 0
            assert lib.svt_amd_picture_ac_energy(ctx, i, energy[i].ctypes.data) == 0
            assert lib.svt_amd_zz_sad_picture(ctx, i, (i - 1) % n, zz[i].ctypes.data) == 0

    arrays = jobs = None
    if form != "blocking":
        arrays = L.DeviceArrays(lib, ctx, n, W, H)
        jobs = L.all_jobs(list(range(n)), first_prev=n - 1)
        host = [np.zeros((n, b), np.uint8) for b in arrays.sizes]

    def batch():
        assert L.launch(lib, ctx, jobs, arrays) == 0, lib.svt_amd_last_error()
        for k in range(6):
            assert lib.svt_amd_device_download(ctx, host[k].ctypes.data, arrays.ptr[k], host[k].size) == 0

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    if form == "blocking":
        blocking(), blocking()
        print(json.dumps({"form": form, "pictures": n, "passes": 2}))
    elif form == "batch":
        batch(), batch()
        print(json.dumps({"form": form, "pictures": n, "passes": 2}))
    else:
        blocking(), batch()                     # code objects, pinned rings, scratch
        got = L.views(host, n, 4, 4)
        same = (got["block_stats"].tobytes() == stats.tobytes() and got["ac_energy"].tobytes() == energy.tobytes() and got["zz"].tobytes() == zz.tobytes()
                and got["histogram"].tobytes() == hist.tobytes() and np.array_equal(got["region_average"][:, :16], ravg) and np.array_equal(got["sum_luma"], total))
        ta, tb = [], []
        for _ in range(5):
            ta.append(timed(blocking))
            tb.append(timed(batch))
        print(json.dumps({"form": form, "pictures": n, "width": W, "height": H, "results_identical": bool(same),
                          "blocking_ms": sorted(ta), "batch_ms": sorted(tb), "blocking_ms_median": float(np.median(ta)), "batch_ms_median": float(np.median(tb))}))
        assert same
    if arrays:
        arrays.free()
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main()
