#!/usr/bin/env python3
"""Device time of svt_amd_md_config_batch_launch for a 64-picture 3840x2160 batch: svt_amd_timer_begin / _end around the call (the descriptor copy, k_mdc_lcu,
k_mdc_budget, k_mdc_leaves) on the context's lane, two warm-up calls, then the median of seven.  The pictures are the job mix of mdc_records._usual_jobs() at
class 3 - P and B pictures of every layer, nine PICT_LCU_SWITCH pictures in twelve, one PICT_FULL85, PICT_FULL84 and PICT_BDP picture - on 64 distinct
seeded record sets.  The split by stage comes from three more timed series with svt_amd_debug_md_config_stages: stage 1 alone, stages 1 + 2, all three; a
stage's share is the difference of two medians, not a measurement of its own.  Prints one JSON line (and writes it to the file given): microseconds per batch,
the split, and the largest pass count of the budgeting loop among the pictures.  Checks two pictures against the restatement (tests/mdc_numpy.py) so that a
number is never reported for wrong results.
usage: md_config_time.py [pictures [output.json]]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import mdc_numpy as N           # noqa: E402
import mdc_records as R         # noqa: E402
import mdclib as M              # noqa: E402
import svtlib as S              # noqa: E402

W, H = 3840, 2160
LAMBDA, SPLIT_BITS = 261, [12171, 78934]
RECORDS = ("me", "stats", "detect", "sbo_lcu", "sbo_pic", "pic_detect", "noise_pic", "stationary_edge")
vp = C.c_void_p


def up(n):
    return (n + 255) & ~255


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    lib = M.declare(S.load_product())
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    nl = S.lcu_count(W, H)
    usual = R._usual_jobs(cls=3)
    jobs_py = [usual[i % len(usual)] for i in range(n)]
    recs = [R.make_inputs(W, H, 70 + i, 0, jb) for i, jb in enumerate(jobs_py)]
    size = sum(up(r[k].nbytes) for r in recs for k in RECORDS if r[k] is not None)
    d_in, d_lcu, d_pic = vp(), vp(), vp()
    for p, b in ((d_in, size), (d_lcu, n * nl * R.MDC_LCU_DTYPE.itemsize), (d_pic, n * R.MDC_PIC_DTYPE.itemsize)):
        assert lib.svt_amd_device_alloc(ctx, b, C.byref(p)) == 0, lib.svt_amd_last_error()
    off, jobs = 0, (M.MdcJob * n)()

    def put(a):
        nonlocal off
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        assert lib.svt_amd_device_upload(ctx, vp(d_in.value + off), a.ctypes.data, a.nbytes) == 0, lib.svt_amd_last_error()
        at, off = d_in.value + off, off + up(a.nbytes)
        return at

    for j, jb, r in zip(jobs, jobs_py, recs):
        for k in RECORDS:
            setattr(j, k, put(r[k]))
        j.cur_slot = -1
        M.fill_scalars(j, jb, LAMBDA, SPLIT_BITS)
    table = M.MdcArrays(d_lcu.value, d_pic.value)

    def series(mask):
        lib.svt_amd_debug_md_config_stages(mask)
        times = []
        for k in range(9):
            ms = C.c_float()
            assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_md_config_batch_launch(ctx, jobs, n, W, H, C.byref(table)) == 0, lib.svt_amd_last_error()
            assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
            if k >= 2:
                times.append(ms.value * 1e3)
        return times

    only_a, a_and_b, whole = series(1), series(3), series(7)      # the whole call last: its records are the ones checked
    lcu, pic = np.zeros((n, nl), R.MDC_LCU_DTYPE), np.zeros(n, R.MDC_PIC_DTYPE)
    assert lib.svt_amd_device_download(ctx, lcu.ctypes.data, d_lcu, lcu.nbytes) == 0
    assert lib.svt_amd_device_download(ctx, pic.ctypes.data, d_pic, pic.nbytes) == 0
    for i in (1, n - 1):
        want_lcu, want_pic, _ = N.md_config(W, H, recs[i], jobs_py[i], LAMBDA, SPLIT_BITS)
        assert lcu[i].tobytes() == want_lcu.tobytes() and pic[i].tobytes() == want_pic.tobytes(), i
    med = lambda t: float(np.median(t))  # noqa: E731
    us = med(whole)
    out = {"pictures": n, "width": W, "height": H, "lcus": nl, "lcu_switch_pictures": int(sum(jb["depth_mode"] == 0 for jb in jobs_py)),
           "us_median": round(us, 1), "us_min": round(min(whole), 1), "us_max": round(max(whole), 1),
           "stages_us": {"k_mdc_lcu": round(med(only_a), 1), "k_mdc_budget": round(med(a_and_b) - med(only_a), 1), "k_mdc_leaves": round(us - med(a_and_b), 1)},
           "series_us": {"stage_1": [round(t, 1) for t in only_a], "stages_1_2": [round(t, 1) for t in a_and_b], "whole": [round(t, 1) for t in whole]},
           "largest_pass_count": int(pic["iterations"].max()), "pass_counts": sorted(set(pic["iterations"].tolist())),
           "beside_us": {"source_ops_batch": 338, "me_batch": 9840}}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")
    for p in (d_in, d_lcu, d_pic):
        lib.svt_amd_device_free(ctx, p)
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main()
