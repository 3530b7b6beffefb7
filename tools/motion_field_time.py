#!/usr/bin/env python3
"""Two measurements of the temporal motion field on the device.
producer: device time of ONE svt_amd_motion_field_launch (k_tmvp_lcu + k_tmvp_stats) for one 3840x2160 picture of seeded work records - svt_amd_timer_begin / _end
around the call on the context's lane, two warm-up calls, then the median of seven - and, beside it, the pair of operations of the mode-decision call it
replaces: hipMemcpyAsync of the LCUs' records from a pageable host array + hipMemsetAsync of the record behind them, between two events on a stream of the HIP
runtime, the same two warm-ups and seven repeats in the same run.  The result is checked against the restatement (tests/tmvp_numpy.py) so that a number is never
reported for wrong results.  Prints one JSON line (and writes it to the file given).
call: wall time of svt_amd_md_encode_picture_inter for one recorded 4K B picture (tools/md_bench.py record_inter, or a .npz of it) with the co-located motion field
as a host array against the same records in device memory, bound with svt_amd_md_picture_set_motion_field: the runs alternate, five each after one warm-up call of
each kind, host calls on one picture object and bound calls on another whose own copy of the field holds zeroes (so that a call which ignored the binding would
decide differently); median and range of both, whether the results were byte-identical, and the condition, reported: the bound median does not exceed the host
median by more than the host series' own spread (max - min without its first call).
usage: motion_field_time.py producer [output.json] | motion_field_time.py call [record.npz [output.txt]]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import svtlib as S              # noqa: E402
import tmvp_numpy as N          # noqa: E402
import tmvplib as T             # noqa: E402

W, H = 3840, 2160
vp = C.c_void_p


def seeded_heads(w, h, seed):
    """quadtrees of 8 to 64 over every LCU, a quarter of the units intra, all three directions"""
    rng = np.random.default_rng(seed)
    wl, hl = (w + 63) // 64, (h + 63) // 64
    heads = np.zeros(wl * hl, T.WORK_HEAD_DTYPE)
    for n in range(wl * hl):
        lw, lh = min(64, w - 64 * (n % wl)), min(64, h - 64 * (n // wl))
        units = []

        def rec(x, y, s):
            if x >= lw or y >= lh:
                return
            if x + s > lw or y + s > lh or (s > 8 and rng.random() < 0.45):
                for dy, dx in ((0, 0), (0, s // 2), (s // 2, 0), (s // 2, s // 2)):
                    rec(x + dx, y + dy, s // 2)
            else:
                units.append((x, y, s))
        rec(0, 0, 64)
        k = len(units)
        cu = heads[n]["cu"]
        heads[n]["num_cus"] = k
        cu["x"][:k], cu["y"][:k], cu["size"][:k] = zip(*units)
        cu["pred_mode"][:k] = np.where(rng.random(k) < 0.25, 2, 1)
        cu["inter_dir"][:k] = rng.integers(0, 3, k)
        cu["mv"][:k] = rng.integers(-2048, 2048, (k, 2, 2))
    return heads


def producer(argv):
    lib = T.declare(S.load_product())
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    nl = S.lcu_count(W, H)
    heads = seeded_heads(W, H, 26)
    raw = np.zeros((nl, T.WORK_BYTES), np.uint8)
    raw[:, :T.LIST_BYTES] = heads.view(np.uint8).reshape(nl, T.LIST_BYTES)
    poc = (8, 16)
    d_works, d_field, d_stats, d_plain = vp(), vp(), vp(), vp()
    for p, b in ((d_works, raw.nbytes), (d_field, (nl + 1) * 416), (d_stats, 256), (d_plain, (nl + 1) * 416)):
        assert lib.svt_amd_device_alloc(ctx, b, C.byref(p)) == 0, lib.svt_amd_last_error()
    assert lib.svt_amd_device_upload(ctx, d_works, raw.ctypes.data, raw.nbytes) == 0, lib.svt_amd_last_error()
    job = T.job(d_works.value, T.WORK_BYTES, W, H, 0, poc)
    times = []
    for k in range(9):
        ms = C.c_float()
        assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_motion_field_launch(ctx, C.byref(job), d_field, d_stats) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
        if k >= 2:
            times.append(ms.value * 1e3)
    got, st = np.zeros(nl + 1, T.TMVP_LCU_DTYPE), np.zeros(1, T.REF_STATS_DTYPE)
    assert lib.svt_amd_device_download(ctx, got.ctypes.data, d_field, got.nbytes) == 0 and lib.svt_amd_device_download(ctx, st.ctypes.data, d_stats, 8) == 0
    want = N.field(heads, W, H, poc)
    assert got.tobytes() == want.tobytes()
    area = N.intra_area_sum(heads)
    assert (int(st[0]["intra_area_sum"]), int(st[0]["intra_coded_area"])) == (area, N.intra_coded_area(area, W, H, 0))

    # what the mode-decision call does with a host field: one copy from pageable memory, one fill, on a stream
    hip = C.CDLL("libamdhip64.so")
    hipMemset = hip.hipMemsetAsync
    for f in (hip.hipStreamCreate, hip.hipEventCreate, hip.hipEventRecord, hip.hipMemcpyAsync, hipMemset, hip.hipEventSynchronize, hip.hipEventElapsedTime,
              hip.hipStreamSynchronize, hip.hipStreamDestroy, hip.hipEventDestroy):
        f.restype = C.c_int
    hip.hipEventRecord.argtypes, hip.hipMemcpyAsync.argtypes = [vp, vp], [vp, vp, C.c_size_t, C.c_int, vp]
    hipMemset.argtypes, hip.hipEventSynchronize.argtypes = [vp, C.c_int, C.c_size_t, vp], [vp]
    hip.hipEventElapsedTime.argtypes, hip.hipStreamSynchronize.argtypes = [C.POINTER(C.c_float), vp, vp], [vp]
    hip.hipStreamDestroy.argtypes, hip.hipEventDestroy.argtypes = [vp], [vp]
    st_, e0, e1 = vp(), vp(), vp()
    assert hip.hipStreamCreate(C.byref(st_)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    host = want[:nl].copy()
    plain = []
    for k in range(9):
        ms = C.c_float()
        assert hip.hipEventRecord(e0, st_) == 0
        assert hip.hipMemcpyAsync(d_plain, host.ctypes.data, nl * 416, 1, st_) == 0
        assert hipMemset(vp(d_plain.value + nl * 416), 0, 416, st_) == 0
        assert hip.hipEventRecord(e1, st_) == 0
        assert hip.hipEventSynchronize(e1) == 0 and hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if k >= 2:
            plain.append(ms.value * 1e3)
    back = np.zeros(nl + 1, T.TMVP_LCU_DTYPE)
    assert lib.svt_amd_device_download(ctx, back.ctypes.data, d_plain, back.nbytes) == 0 and back.tobytes() == want.tobytes()
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1), hip.hipStreamDestroy(st_)

    def stats(t):
        return {"us_median": round(float(np.median(t)), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1), "series_us": [round(v, 1) for v in t]}
    out = {"width": W, "height": H, "lcus": nl, "units": int(heads["num_cus"].sum()), "available_units": int(want["available"].sum()),
           "intra_coded_area": int(st[0]["intra_coded_area"]), "bytes_written": (nl + 1) * 416 + 8, "producer": stats(times),
           "copy_and_fill_it_replaces": stats(plain)}
    line = json.dumps(out)
    print(line)
    if argv:
        with open(argv[0], "w") as f:
            f.write(line + "\n")
    for p in (d_works, d_field, d_stats, d_plain):
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
    lib = T.declare(S.load_product())
    from test_gpu_md import sig
    sig(lib)
    lib.svt_amd_md_encode_picture_inter.restype = C.c_int
    lib.svt_amd_md_encode_picture_inter.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_set_inter.restype, lib.svt_amd_encdec_picture_set_inter.argtypes = C.c_int, [vp] * 5
    k = next(i for i in range(len(g["picture_number"])) if g["tmvp_present"][i] and g["inter"][i]["tmvp_enable"] and g["tmvp"][i]["available"].any())
    w, h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
    ctx, d_field = vp(), vp()
    pics = {False: vp(), True: vp()}   # host calls and bound calls on a picture object each: the bound one never uploads the recorded field itself
    assert lib.svt_amd_context_create(0, w, (h + 7) & ~7, 2, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    for pic in pics.values():
        assert lib.svt_amd_encdec_picture_create(ctx, w, h, 1, C.byref(pic)) == 0, lib.svt_amd_last_error()
    P, lcus, cost, ois = (np.ascontiguousarray(a) for a in (g["pic"][k:k + 1], g["lcu"][k], g["cost"][k], g["ois"][k]))
    src = [np.ascontiguousarray(g[nm][k]) for nm in ("src_y", "src_cb", "src_cr")]
    X, me, tmvp, refs, planes = inter_inputs(g, k)
    dev = [[torch.from_numpy(a).cuda() for a in pl] for pl in planes]
    torch.cuda.synchronize()
    rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r.strideY, r.strideC, r.originX, r.originY, r.width, r.height) for d, r in zip(dev, refs)]
    for pic in pics.values():
        assert lib.svt_amd_encdec_picture_set_inter(ctx, pic, C.byref(rs[0]), C.byref(rs[1]), cost.ctypes.data) == 0, lib.svt_amd_last_error()
    n = len(lcus)
    field = np.zeros(n + 1, T.TMVP_LCU_DTYPE)
    field[:n] = tmvp
    assert lib.svt_amd_device_alloc(ctx, field.nbytes, C.byref(d_field)) == 0 and lib.svt_amd_device_upload(ctx, d_field, field.ctypes.data, field.nbytes) == 0
    out, works, res = np.zeros(n, S.MD_LCU_OUT_DTYPE), np.zeros(n, S.LCU_WORK_DTYPE), np.zeros(n, S.LCU_RESULT_DTYPE)

    def one(bound, host_field=None):
        pic = pics[bound]
        if bound and host_field is None:
            assert lib.svt_amd_md_picture_set_motion_field(ctx, pic, d_field) == 0
        host_field = host_field if host_field is not None else None if bound else tmvp
        t0 = time.perf_counter()
        rc = lib.svt_amd_md_encode_picture_inter(ctx, pic, P.ctypes.data, X.ctypes.data, lcus.ctypes.data, src[0].ctypes.data, src[0].shape[1], src[1].ctypes.data,
                                                 src[2].ctypes.data, src[1].shape[1], ois.ctypes.data, 0, me.ctypes.data, 0,
                                                 host_field.ctypes.data if host_field is not None else None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, lib.svt_amd_last_error()
        return ms, (out.tobytes(), works.tobytes(), res.tobytes())

    from test_gpu_mdctl_batch import decisions   # the bytes of md_out the call defines: the fields of untested leaves are the workgroups' LDS leftovers

    def key(r):
        a = np.frombuffer(decisions(r[0]), S.MD_LCU_OUT_DTYPE).copy()
        a["pad"] = 0   # never written by the kernel: what the picture object's allocation held, and the two kinds of call run on two objects
        return a.tobytes(), r[1], r[2]
    _, want = one(False)
    # the bound calls' object uploads a ZERO field of its own first: a call that ignored the binding would read that one again, and decide differently
    _, blind = one(True, host_field=np.zeros(n, T.TMVP_LCU_DTYPE))
    field_matters = key(blind) != key(want)
    _, got = one(True)
    identical = key(want) == key(got)
    ts = {False: [], True: []}
    for rep in range(5):
        for bound in (False, True):
            ms, b = one(bound)
            identical = identical and key(b) == key(want)
            ts[bound].append(ms)
    lines = ["# svt_amd_md_encode_picture_inter, one %dx%d B picture (%d LCUs, temporal layer %d, %d available units in its co-located field), wall ms of the blocking call, "
             "runs alternated, 5 each after a warm-up of each" % (w, h, n, int(P["temporal_layer"][0]), int(tmvp["available"].sum()))]
    for bound, name in ((False, "host tmvp (the parent's path: %d-byte upload + fill)" % (n * 416)), (True, "bound device field (read in place)")):
        t = ts[bound]
        lines.append("%-60s median %.3f  min %.3f  max %.3f  series %s" % (name, float(np.median(t)), min(t), max(t), " ".join("%.3f" % v for v in t)))
    diff, spread = float(np.median(ts[True])) - float(np.median(ts[False])), max(ts[False][1:]) - min(ts[False][1:])
    lines.append("difference of the medians (bound - host): %+.3f ms; spread of the host series without its first call (max - min): %.3f ms; condition (difference <= spread): %s"
                 % (diff, spread, "met" if diff <= spread else "NOT met"))
    lines.append("no gain is claimed from one run: a difference counts only beyond the spread, and then only when it repeats")
    lines.append("decisions (every defined byte of md_out), work records and results byte-identical in all 12 calls: %s; the bound calls ran on a picture object whose own "
                 "copy held a zero field, which decides differently from the recorded one: %s" % (identical, field_matters))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(argv) > 1:
        with open(argv[1], "w") as f:
            f.write(text)
    del dev
    lib.svt_amd_device_free(ctx, d_field)
    for pic in pics.values():
        lib.svt_amd_encdec_picture_destroy(ctx, pic)
    lib.svt_amd_context_destroy(ctx)
    assert identical and field_matters   # (the timing condition is reported, not asserted: a measuring script does not fail on noise)


if __name__ == "__main__":
    {"producer": producer, "call": call}[sys.argv[1] if len(sys.argv) > 1 else "producer"](sys.argv[2:])
