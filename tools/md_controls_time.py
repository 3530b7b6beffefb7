#!/usr/bin/env python3
"""Two measurements of the mode-decision LCU controls on the device.
batch: device time of svt_amd_md_controls_batch_launch for a 64-picture 3840x2160 batch - svt_amd_timer_begin / _end around ONE call (the descriptor copy and
k_mdctl_lcu) on the context's lane, two warm-up calls, then the median of seven.  The pictures are 64 distinct seeded record sets of mdctl_records at class 3 under
its usual jobs (every chroma level, with and without configuration records and initial-rate-control records), 6 x 4 tiles.  Pictures 1 and 63 are checked against
the restatement (tests/mdctl_numpy.py) so that a number is never reported for wrong results.  Prints one JSON line (and writes it to the file given).
call: wall time of svt_amd_md_encode_picture_inter for one recorded 4K B picture (tools/md_bench.py record_inter, the at-scale path; a .npz of it may be given) with
the controls as a host array against the same records in device memory and bound with svt_amd_md_picture_set_controls: the runs alternate, five each after one
warm-up call of each kind; median and range of both, and whether the decisions were byte-identical.
usage: md_controls_time.py batch [pictures [output.json]] | md_controls_time.py call [record.npz [output.txt]]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import mdctl_numpy as N         # noqa: E402
import mdctl_records as R       # noqa: E402
import mdctllib as M            # noqa: E402
import svtlib as S              # noqa: E402

W, H, CLS, TILES = 3840, 2160, 3, (6, 4)
vp = C.c_void_p


def up(n):
    return (n + 255) & ~255


def batch(argv):
    n = int(argv[0]) if argv else 64
    lib = M.declare(S.load_product())
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    nl = S.lcu_count(W, H)
    usual = R._usual_jobs(CLS, TILES)
    jobs_py = [usual[i % len(usual)] for i in range(n)]
    recs = [R.make_inputs(W, H, 90, i, jb) for i, jb in enumerate(jobs_py)]
    d_in, d_out = vp(), vp()
    for p, b in ((d_in, sum(up(r[k].nbytes) for r in recs for k in M.POINTER_FIELDS if r[k] is not None)), (d_out, n * nl * 191)):
        assert lib.svt_amd_device_alloc(ctx, b, C.byref(p)) == 0, lib.svt_amd_last_error()
    off, jobs, read_bytes = 0, (M.MdCtlJob * n)(), 0
    for j, jb, r in zip(jobs, jobs_py, recs):
        at = {}
        for k in M.POINTER_FIELDS:
            at[k] = None
            if r[k] is not None:
                a = np.ascontiguousarray(r[k])
                assert lib.svt_amd_device_upload(ctx, vp(d_in.value + off), a.ctypes.data, a.nbytes) == 0, lib.svt_amd_last_error()
                at[k], off = d_in.value + off, off + up(a.nbytes)
                read_bytes += a.nbytes
        M.fill_job(j, jb, lambda kind: at[kind])
    times = []
    for k in range(9):
        ms = C.c_float()
        assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_md_controls_batch_launch(ctx, jobs, n, W, H, d_out) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
        if k >= 2:
            times.append(ms.value * 1e3)
    got = np.zeros((n, nl), R.MD_LCU_DTYPE)
    assert lib.svt_amd_device_download(ctx, got.ctypes.data, d_out, got.nbytes) == 0
    for i in (1, n - 1):
        assert got[i].tobytes() == N.md_controls(W, H, recs[i], jobs_py[i]).tobytes(), i
    out = {"pictures": n, "width": W, "height": H, "lcus": nl, "us_median": round(float(np.median(times)), 1), "us_min": round(min(times), 1),
           "us_max": round(max(times), 1), "series_us": [round(t, 1) for t in times], "bytes_written": n * nl * 191, "record_bytes_uploaded": read_bytes,
           "chroma_modes": np.bincount(got["chroma_encode_mode"].ravel(), minlength=3)[1:].tolist(),
           "contouring_classes": np.bincount(got["contouring_class"].ravel(), minlength=4).tolist()}
    line = json.dumps(out)
    print(line)
    if len(argv) > 1:
        with open(argv[1], "w") as f:
            f.write(line + "\n")
    for p in (d_in, d_out):
        lib.svt_amd_device_free(ctx, p)
    lib.svt_amd_context_destroy(ctx)


def call(argv):
    import torch
    from test_oracle_md_golden import inter_inputs
    if argv:
        g = np.load(argv[0])
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from md_bench import record_inter
        g = record_inter(W, H, 8, frames=9, kind="objects", levels=3)
    lib = M.declare(S.load_product())
    from test_gpu_md import sig
    sig(lib)
    lib.svt_amd_md_encode_picture_inter.restype = C.c_int
    lib.svt_amd_md_encode_picture_inter.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_set_inter.restype, lib.svt_amd_encdec_picture_set_inter.argtypes = C.c_int, [vp] * 5
    k = 0
    w, h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
    ctx, pic, d_lcus = vp(), vp(), vp()
    assert lib.svt_amd_context_create(0, w, (h + 7) & ~7, 2, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    assert lib.svt_amd_encdec_picture_create(ctx, w, h, 1, C.byref(pic)) == 0, lib.svt_amd_last_error()
    P, lcus, cost, ois = (np.ascontiguousarray(a) for a in (g["pic"][k:k + 1], g["lcu"][k], g["cost"][k], g["ois"][k]))
    src = [np.ascontiguousarray(g[nm][k]) for nm in ("src_y", "src_cb", "src_cr")]
    X, me, tmvp, refs, planes = inter_inputs(g, k)
    dev = [[torch.from_numpy(a).cuda() for a in pl] for pl in planes]
    torch.cuda.synchronize()
    rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r.strideY, r.strideC, r.originX, r.originY, r.width, r.height) for d, r in zip(dev, refs)]
    assert lib.svt_amd_encdec_picture_set_inter(ctx, pic, C.byref(rs[0]), C.byref(rs[1]), cost.ctypes.data) == 0, lib.svt_amd_last_error()
    n = len(lcus)
    assert lib.svt_amd_device_alloc(ctx, lcus.nbytes, C.byref(d_lcus)) == 0 and lib.svt_amd_device_upload(ctx, d_lcus, lcus.ctypes.data, lcus.nbytes) == 0
    out, works, res = np.zeros(n, S.MD_LCU_OUT_DTYPE), np.zeros(n, S.LCU_WORK_DTYPE), np.zeros(n, S.LCU_RESULT_DTYPE)

    def one(bound):
        if bound:
            assert lib.svt_amd_md_picture_set_controls(ctx, pic, d_lcus) == 0
        t0 = time.perf_counter()
        rc = lib.svt_amd_md_encode_picture_inter(ctx, pic, P.ctypes.data, X.ctypes.data, None if bound else lcus.ctypes.data, src[0].ctypes.data, src[0].shape[1],
                                                 src[1].ctypes.data, src[2].ctypes.data, src[1].shape[1], ois.ctypes.data, 0, me.ctypes.data, 0,
                                                 tmvp.ctypes.data if tmvp is not None else None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, lib.svt_amd_last_error()
        return ms, (out.tobytes(), works.tobytes(), res.tobytes())

    from test_gpu_mdctl_batch import decisions   # the bytes of md_out the call defines: the fields of untested leaves are the workgroups' LDS leftovers

    def key(r):
        return decisions(r[0]), r[1], r[2]
    _, want = one(False)
    _, got = one(True)
    identical = key(want) == key(got)
    ts = {False: [], True: []}
    for rep in range(5):
        for bound in (False, True):
            ms, b = one(bound)
            identical = identical and key(b) == key(want)
            ts[bound].append(ms)
    lines = ["# svt_amd_md_encode_picture_inter, one %dx%d B picture (%d LCUs, temporal layer %d), wall ms of the blocking call, runs alternated, 5 each after a warm-up of each"
             % (w, h, n, int(P["temporal_layer"][0]))]
    for bound, name in ((False, "host lcus (the parent's path: loop over the LCUs + upload)"), (True, "bound device array (check kernel + 88-byte copy + one synchronisation)")):
        t = ts[bound]
        lines.append("%-72s median %.3f  min %.3f  max %.3f  series %s" % (name, float(np.median(t)), min(t), max(t), " ".join("%.3f" % v for v in t)))
    lines.append("difference of the medians (bound - host): %+.3f ms; decisions (every defined byte of md_out), work records and results byte-identical in all 12 calls: %s"
                 % (float(np.median(ts[True])) - float(np.median(ts[False])), identical))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(argv) > 1:
        with open(argv[1], "w") as f:
            f.write(text)
    del dev
    lib.svt_amd_device_free(ctx, d_lcus)
    lib.svt_amd_encdec_picture_destroy(ctx, pic)
    lib.svt_amd_context_destroy(ctx)
    assert identical


if __name__ == "__main__":
    {"batch": batch, "call": call}[sys.argv[1] if len(sys.argv) > 1 else "batch"](sys.argv[2:])
