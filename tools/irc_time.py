#!/usr/bin/env python3
"""Device time of svt_amd_initial_rc_batch_launch for a 64-picture 3840x2160 batch: svt_amd_timer_begin / _end around ONE call (the descriptor copy, k_irc_lcu,
k_irc_motion, k_irc_counts, k_irc_finish) on the context's lane, two warm-up calls, then the median of seven.  The pictures are one 64-picture sequence of
irc_records - I, P and B pictures of four layers, pan, tilt, still and mixed motion, a 17-picture look-ahead whose windows lie inside the batch, the sequence
end in its last pictures - on 64 distinct seeded record sets at class 3.  Prints one JSON line (and writes it to the file given): microseconds per batch.
Checks pictures 1 and 63 against the restatement (tests/irc_numpy.py) so that a number is never reported for wrong results.
usage: irc_time.py [pictures [output.json]]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import irc_numpy as N           # noqa: E402
import irc_records as R         # noqa: E402
import irclib as M              # noqa: E402
import svtlib as S              # noqa: E402

W, H, CLS = 3840, 2160, 3
KINDS = ("checks", "motion", "lcu", "stationary_edge", "pm_stationary_edge", "picture")
vp = C.c_void_p


def up(n):
    return (n + 255) & ~255


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    lib = M.declare(S.load_product())
    ctx = vp()
    assert lib.svt_amd_context_create(0, W, H, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    nl = S.lcu_count(W, H)
    seq = R.sequence(R._run(n, "pppppppptttmsppp", scene_at=(20,), intra_at=(32,), p_at=(8, 40)), lad=17, period=8, head0=R.QUEUE_DEPTH - 30)
    recs = R.make_inputs(W, H, CLS, 80, seq)
    lists = N.sequence_lists(seq)
    sizes = [lib.svt_amd_initial_rc_bytes(W, H, which) for which in range(6)]
    d_in, d_out = vp(), [vp() for _ in KINDS]
    for p, b in [(d_in, sum(up(r[k].nbytes) for r in recs for k in ("me", "stats", "detect")))] + [(p, n * b) for p, b in zip(d_out, sizes)]:
        assert lib.svt_amd_device_alloc(ctx, b, C.byref(p)) == 0, lib.svt_amd_last_error()
    off, where = 0, []
    for r in recs:
        at = {}
        for k in ("me", "stats", "detect"):
            a = np.ascontiguousarray(r[k])
            assert lib.svt_amd_device_upload(ctx, vp(d_in.value + off), a.ctypes.data, a.nbytes) == 0, lib.svt_amd_last_error()
            at[k], off = d_in.value + off, off + up(a.nbytes)
        where.append(at)
    jobs = (M.IrcJob * n)()

    def at(kind, k):
        return where[k][kind] if kind in ("stats", "detect") else d_out[KINDS.index(kind)].value + k * sizes[KINDS.index(kind)]

    for i, j in enumerate(jobs):
        j.me, j.stats, j.cur_slot = where[i]["me"], where[i]["stats"], -1
        M.fill_job(j, seq["pics"][i], CLS, lists[i], at)
    table = M.IrcArrays(*[p.value for p in d_out])
    times = []
    for k in range(9):
        ms = C.c_float()
        assert lib.svt_amd_timer_begin(ctx) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_initial_rc_batch_launch(ctx, jobs, n, W, H, C.byref(table)) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_timer_end(ctx, C.byref(ms)) == 0, lib.svt_amd_last_error()
        if k >= 2:
            times.append(ms.value * 1e3)
    got = {}
    for kind, p, b in zip(KINDS, d_out, sizes):
        got[kind] = np.zeros((n, b), np.uint8)
        assert lib.svt_amd_device_download(ctx, got[kind].ctypes.data, p, got[kind].nbytes) == 0
    checked = (1, n - 1)
    want = N.initial_rc(W, H, CLS, seq, recs, lists, only=checked)
    for i in checked:
        for kind in KINDS:
            w = np.ascontiguousarray(want[kind][i]).view(np.uint8).ravel()
            assert got[kind][i, :w.size].tobytes() == w.tobytes() and not got[kind][i, w.size:].any(), (i, kind)
    flags = got["stationary_edge"][:, :nl]
    out = {"pictures": n, "width": W, "height": H, "lcus": nl, "us_median": round(float(np.median(times)), 1), "us_min": round(min(times), 1),
           "us_max": round(max(times), 1), "series_us": [round(t, 1) for t in times], "stationary_lcus": np.bincount(flags.ravel(), minlength=4).tolist(),
           "look_ahead_pictures": int(sum(ls["look_ahead"] for ls in lists))}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")
    for p in [d_in] + d_out:
        lib.svt_amd_device_free(ctx, p)
    lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    main()
