#!/usr/bin/env python3
"""Device time of svt_amd_noise_detect_batch_launch for a 64-picture 3840x2160 batch, per method: svt_amd_timer_begin / _end around the call (the two fills, the
descriptor copy, k_noise_blocks, k_noise_finish), two warm-up calls, then the median of seven.  Prints one JSON line: microseconds per batch, the bytes of the
planes the method reads (the algorithmic bytes) and the rate they make.  Checks two pictures of every batch against the numpy restatement
(tests/pa_noise_numpy.py) so that a number is never reported for wrong results.
usage: noise_detect_time.py [pictures]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pa_noise_numpy as N      # noqa: E402
import pa_noise_pictures as P   # noqa: E402
import svtlib as S              # noqa: E402

W, H = 3840, 2160
vp = C.c_void_p


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    lib = N.declare(S.load_product())
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, n, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    base = [P.picture(W, H, P.spec(40 + i, a, ramp=(0, 16)[i & 1])) for i, a in enumerate((0, 6, 14, 30))]
    frames = [np.ascontiguousarray(np.roll(base[i % 4], (3 * (i // 4), 5 * (i // 4)), (0, 1))) for i in range(n)]
    for i, f in enumerate(frames):
        assert lib.svt_amd_picture_upload(ctx, i, f.ctypes.data, W, W, H) == 0, lib.svt_amd_last_error()
    sizes = N.sizes(W, H)
    d = [vp(), vp()]
    for p, b in zip(d, sizes):
        assert lib.svt_amd_device_alloc(ctx, n * b, C.byref(p)) == 0, lib.svt_amd_last_error()
    table = N.NoiseArrays(d[0].value, d[1].value)
    out = {"pictures": n, "width": W, "height": H}
    for method, shift in ((N.FULL, 0), (N.QUARTER, 1), (N.HALF, 2)):
        jobs = N.make_jobs([(i, method, i & 1) for i in range(n)])
        times = []
        for k in range(9):
            ms = C.c_float()
            assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_noise_detect_batch_launch(ctx, jobs, n, C.byref(table)) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
            if k >= 2:
                times.append(ms.value * 1e3)
        flat, pic = np.zeros((n, sizes[0]), np.uint8), np.zeros(n, N.PIC_DTYPE)
        assert lib.svt_amd_device_download(ctx, flat.ctypes.data, d[0], flat.size) == 0
        assert lib.svt_amd_device_download(ctx, pic.ctypes.data, d[1], pic.nbytes) == 0
        for i in (1, n - 1):
            want_flat, want_pic = N.detect(frames[i], method, i & 1)
            assert np.array_equal(flat[i], want_flat) and pic[i].tobytes() == want_pic.tobytes(), (P.METHOD_NAME[method], i, pic[i], want_pic)
        plane_bytes = n * (W >> shift) * (H >> shift)
        us = float(np.median(times))
        out[P.METHOD_NAME[method]] = {"us_median": round(us, 1), "us_min": round(min(times), 1), "us_max": round(max(times), 1), "plane_bytes": plane_bytes,
                                      "tb_per_s": round(plane_bytes / us / 1e6, 3), "classes": sorted(set(int(c) for c in pic["pic_noise_class"])),
                                      "flagged_lcus": int(flat.sum())}
    print(json.dumps(out))
    for p in d:
        lib.svt_amd_device_free(ctx, p)
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main()
