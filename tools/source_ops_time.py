#!/usr/bin/env python3
"""Device time of svt_amd_source_ops_batch_launch for a 64-picture 3840x2160 batch: svt_amd_timer_begin / _end around the call (the descriptor copy, k_sbo_lcu,
k_sbo_finish), two warm-up calls, then the median of seven.  Two batches: `records` - I / P / B pictures that all want the QPM statistics, so every picture
reads its ME and OIS records (64 distinct record sets, 1.3 GB: more than the caches hold) - and `plain` - the same pictures as I pictures without want_qpm, which
read neither.  Prints one JSON line: microseconds per batch and the bytes of the cache lines the kernels touch.  Checks two pictures of every batch against the
restatement (tests/sbo_numpy.py) so that a number is never reported for wrong results.
usage: source_ops_time.py [pictures]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sbo_numpy as N           # noqa: E402
import sbo_records as R         # noqa: E402
import svtlib as S              # noqa: E402

W, H, RW, RH = 3840, 2160, 4, 4
RECORDS = ("stats", "ref_stats", "chroma", "detect", "histogram", "me", "ois")
vp = C.c_void_p


def up(n):
    return (n + 255) & ~255


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    lib = R.declare(S.load_product())
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    nl = S.lcu_count(W, H)
    kinds = [R.job(R.I, 0, 1, 17, qpm=1, hist="dark"), R.job(R.P, 0, 1, 17, qpm=1, activity="active"), R.job(R.B, 1, 1, 17, qpm=1, skip=1, cls=3, activity="active"),
             R.job(R.B, 2, 0, 17, qpm=1, cls=3, activity="moderate")]
    jobs_py = [dict(kinds[i % 4], cls=3) for i in range(n)]
    recs = [R.make_inputs(W, H, RW, RH, 50 + i, 0, jb) for i, jb in enumerate(jobs_py)]
    size = sum(up(r[k].nbytes) for r in recs for k in RECORDS) + sum(up(z.nbytes) for r in recs for z in r["zz"])
    d_in, d_lcu, d_pic = vp(), vp(), vp()
    for p, b in ((d_in, size), (d_lcu, n * nl * R.SBO_LCU_DTYPE.itemsize), (d_pic, n * R.SBO_PIC_DTYPE.itemsize)):
        assert lib.svt_amd_device_alloc(ctx, b, C.byref(p)) == 0, lib.svt_amd_last_error()
    off, jobs = 0, (R.SboJob * n)()

    def put(a):
        nonlocal off
        a = np.ascontiguousarray(a)
        assert lib.svt_amd_device_upload(ctx, vp(d_in.value + off), a.ctypes.data, a.nbytes) == 0, lib.svt_amd_last_error()
        at, off = d_in.value + off, off + up(a.nbytes)
        return at

    for j, jb, r in zip(jobs, jobs_py, recs):
        j.stats, j.ref_stats, j.chroma, j.detect, j.histogram, j.me, j.ois = (put(r[k]) for k in RECORDS)
        for k, z in enumerate(r["zz"]):
            j.zz[k] = put(z)
        j.cur_slot, j.zz_count, j.slice_type, j.temporal_layer_index, j.is_used_as_reference = -1, jb["zz_count"], jb["slice_type"], jb["layer"], jb["ref"]
        j.resolution_class, j.skip_ois_8x8, j.cu8x8_mode, j.want_qpm = jb["cls"], jb["skip"], jb["cu8"], jb["qpm"]
    table = R.SboArrays(d_lcu.value, d_pic.value)
    out = {"pictures": n, "width": W, "height": H, "lcus": nl}
    for name in ("records", "plain"):
        if name == "plain":
            for j, jb in zip(jobs, jobs_py):
                j.slice_type, j.want_qpm, j.ref_stats = 0, 0, None
                jb.update(slice_type=0, qpm=0)
        times = []
        for k in range(9):
            ms = C.c_float()
            assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_source_ops_batch_launch(ctx, jobs, n, W, H, RW, RH, C.byref(table)) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
            if k >= 2:
                times.append(ms.value * 1e3)
        lcu, pic = np.zeros((n, nl), R.SBO_LCU_DTYPE), np.zeros(n, R.SBO_PIC_DTYPE)
        assert lib.svt_amd_device_download(ctx, lcu.ctypes.data, d_lcu, lcu.nbytes) == 0
        assert lib.svt_amd_device_download(ctx, pic.ctypes.data, d_pic, pic.nbytes) == 0
        for i in (1, n - 1):
            rec = recs[i] if jobs_py[i]["slice_type"] else dict(recs[i], ref_stats=None)
            want_lcu, want_pic, _ = N.source_ops(W, H, rec, jobs_py[i])
            assert lcu[i].tobytes() == want_lcu.tobytes() and pic[i].tobytes() == want_pic.tobytes(), (name, i)
        # the cache lines touched per LCU: the statistics, chroma and detector records and 17 zz records; with the records the ME units' 24-byte entries
        # (2040 contiguous bytes) and every 72-byte candidate row of the OIS record (6120 bytes)
        touched = n * nl * (256 + 48 + 48 + 17 * 8 + 24 + (2040 + 6120 if name == "records" else 0))
        us = float(np.median(times))
        out[name] = {"us_median": round(us, 1), "us_min": round(min(times), 1), "us_max": round(max(times), 1), "touched_bytes": touched,
                     "tb_per_s": round(touched / us / 1e6, 3)}
    print(json.dumps(out))
    for p in (d_in, d_lcu, d_pic):
        lib.svt_amd_device_free(ctx, p)
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main()
