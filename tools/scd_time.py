#!/usr/bin/env python3
"""Device time of svt_amd_scene_detect_batch_launch for a 64-job batch at 3840x2160 with 4 x 4 regions: svt_amd_timer_begin / _end around ONE call (the
descriptor copy, k_scd_ahd, k_scd_decide) on the context's lane, two warm-up calls, then the median of seven - for the whole entry, for k_scd_ahd alone, for
k_scd_decide alone and for the descriptor copy alone (svt_amd_debug_scene_detect_stages; every figure holds the copy and the timer's two events).  Beside it, in the same run, what the entry makes
unnecessary: svt_amd_device_download_async + svt_amd_synchronize of the 64 x 48 KB of histograms into pinned host memory, by the same device timer and by the
host's clock, and the host's clock for the download of the 64 picture records the entry leaves instead.  The records are a seeded script of
tests/scd_records.py; the results are checked against the restatement (tests/scd_numpy.py) so that a number is never reported for wrong results.
Prints one JSON line (and writes it to the file given).
usage: scd_time.py [jobs [output.json]]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import scd_numpy as N           # noqa: E402
import scd_records as R         # noqa: E402
import scdlib as M              # noqa: E402
import svtlib as S              # noqa: E402

W, H, RW, RH, MODE, SEED = 3840, 2160, 4, 4, 1, 120
PARTS = ("luma", "chroma", "avg", "detect")
KINDS = ("picture", "ahd", "state")
vp = C.c_void_p


def up(n):
    return (n + 255) & ~255


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    lib = M.declare(S.load_product())
    lib.svt_amd_device_alloc.argtypes = lib.svt_amd_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.svt_amd_device_upload.argtypes = lib.svt_amd_device_download.argtypes = lib.svt_amd_device_download_async.argtypes = [vp, vp, vp, C.c_size_t]
    lib.svt_amd_device_free.argtypes = lib.svt_amd_host_free.argtypes = [vp, vp]
    ctx = vp()
    assert lib.svt_amd_context_create(0, 64, 64, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    pics = R.Script(W, H, RW, RH, SEED).run(n, R.long_events(n, SEED))
    windows = [R.window(pics, i) for i in range(n)]
    sizes = [lib.svt_amd_scene_detect_bytes(which, RW, RH) for which in range(3)]
    d_in, d_out = vp(), [vp() for _ in KINDS]
    for p, b in [(d_in, sum(up(pic[k].nbytes) for pic in pics for k in PARTS))] + [(p, n * b) for p, b in zip(d_out, sizes)]:
        assert lib.svt_amd_device_alloc(ctx, b, C.byref(p)) == 0, lib.svt_amd_last_error()
    off, where, keep = 0, [], []
    for pic in pics:
        at = {}
        for k in PARTS:
            a = np.ascontiguousarray(pic[k])
            keep.append(a)
            assert lib.svt_amd_device_upload(ctx, vp(d_in.value + off), a.ctypes.data, a.nbytes) == 0, lib.svt_amd_last_error()
            at[k], off = d_in.value + off, off + up(a.nbytes)
        where.append(at)
    jobs = (M.ScdJob * n)()
    for i, j in enumerate(jobs):
        past, cur, future = where[i], where[i + 1], where[i + 2]
        j.past_histogram, j.cur_histogram, j.past_chroma_histogram, j.cur_chroma_histogram = past["luma"], cur["luma"], past["chroma"], cur["chroma"]
        j.past_region_average, j.cur_region_average, j.future_region_average = past["avg"], cur["avg"], future["avg"]
        j.past_detect, j.cur_detect = past["detect"], cur["detect"]
    table = M.ScdArrays(*[p.value for p in d_out])

    def timed(call):
        """two warm-up calls, then seven: (device microseconds, host microseconds up to the end of the timer's wait)"""
        dev, host = [], []
        for k in range(9):
            ms = C.c_float()
            t0 = time.perf_counter()
            assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
            call()
            assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
            if k >= 2:
                dev.append(ms.value * 1e3), host.append((time.perf_counter() - t0) * 1e6)
        return dev, host

    def entry():
        assert lib.svt_amd_scene_detect_batch_launch(ctx, jobs, n, W, H, RW, RH, MODE, None, C.byref(table)) == 0, lib.svt_amd_last_error()

    series = {}
    try:
        for name, mask in (("entry", 3), ("ahd_only", 1), ("decide_only", 2), ("descriptor_copy_only", 0)):
            lib.svt_amd_debug_scene_detect_stages(mask)
            series[name] = timed(entry)[0]
    finally:
        lib.svt_amd_debug_scene_detect_stages(3)    # the mask is the process's: whatever happens, both stages run again
    entry()
    got = {}
    for kind, p, b in zip(KINDS, d_out, sizes):
        got[kind] = np.zeros((n, b), np.uint8)
        assert lib.svt_amd_device_download(ctx, got[kind].ctypes.data, p, got[kind].nbytes) == 0
    want = N.scene_detect(W, H, RW, RH, MODE, windows)
    R.same(dict(picture=got["picture"].view(R.PIC_DTYPE)[:, 0], ahd=got["ahd"].view(R.AHD_DTYPE).reshape(n, 16, 3), state=got["state"].view(R.STATE_DTYPE)[:, 0]),
           want, "scd_time")

    # what the entry makes unnecessary: the histograms of the n pictures to the host, 48 KB each (luma 16 KB + chroma 32 KB), one copy
    hist_bytes = n * 16 * 3 * 1024
    d_hist, h_hist, h_pic = vp(), vp(), vp()
    assert lib.svt_amd_device_alloc(ctx, hist_bytes, C.byref(d_hist)) == 0, lib.svt_amd_last_error()
    assert lib.svt_amd_host_alloc(ctx, hist_bytes, C.byref(h_hist)) == 0 and lib.svt_amd_host_alloc(ctx, n * sizes[0], C.byref(h_pic)) == 0, lib.svt_amd_last_error()

    def download(dst, src, nbytes):
        def call():
            assert lib.svt_amd_device_download_async(ctx, dst, src, nbytes) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_synchronize(ctx) == 0, lib.svt_amd_last_error()
        return call
    hist_dev, hist_host = timed(download(h_hist, d_hist, hist_bytes))
    _, pic_host = timed(download(h_pic, d_out[0], n * sizes[0]))

    def stats(t):
        return {"us_median": round(float(np.median(t)), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}
    out = {"jobs": n, "width": W, "height": H, "regions": [RW, RH], "scene_changes": int(want["picture"]["scene_change"].sum()),
           "resets": int(want["picture"]["reset_running_avg"].sum())}
    out.update({k: stats(v) for k, v in series.items()})
    out["histogram_download"] = dict(bytes=hist_bytes, device=stats(hist_dev), host=stats(hist_host))
    out["picture_record_download"] = dict(bytes=n * sizes[0], host=stats(pic_host))
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")
    lib.svt_amd_host_free(ctx, h_hist), lib.svt_amd_host_free(ctx, h_pic)
    for p in [d_in, d_hist] + d_out:
        lib.svt_amd_device_free(ctx, p)
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main()
