#!/usr/bin/env python3
"""GPU box: what svt_amd_md_encode_picture_launch costs the host against the blocking call, and the chain of tests/test_gpu_md_launch.py (q -> tail -> motion field ->
controls -> p on one lane) against the same chain with blocking mode-decision calls.  One JSON line per mode.
usage: md_launch_time.py host     host time inside the call and call -> completed results, launch against blocking, five each, alternated: the 1080p I fixture and
                                  picture 0 of the recorded 4K B pictures (tools/_fx/md4k.npz, tools/md_record_4k.py)
       md_launch_time.py chain    first call -> completed results of the chain (md_bref / md_b_motion_416x240_m8, pictures 2 -> 3), five each, alternated
       md_launch_time.py source   three launches and three blocking calls of a 3840x2160 picture at 8 and at 10 bits, for a kernel trace around the process
                                  (k_md_source against the copy + k_msb_view of the blocking call)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mdlaunchlib as M
import svtlib as S
import taillib
import tmvplib as T
from pa_batch_util import DeviceBuffer, make_context, ok
from test_gpu_mdctl_batch import Out, Pictures, _md_sig, launch as controls_launch, same_call

FIELD_REC = T.TMVP_LCU_DTYPE.itemsize
FX_4K = os.path.join(ROOT, "tools", "_fx", "md4k.npz")

REPS = 5


class G(dict):
    files = property(lambda self: list(self.keys()))


def library():
    lib = S.load_product()
    _md_sig(lib)
    return taillib.declare(T.declare(M.declare(lib)))


def ms(v):
    return [round(1e3 * x, 3) for x in v]


def host_times(lib, g, k, tag):
    w, h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
    ctx = make_context(lib, w, (h + 7) & ~7, 2)
    obj = M.Obj(lib, ctx, g, k)
    inp = obj.inputs()
    job = M.make_job(obj, inp, M.tiles_of(obj.lcus))
    ok(lib, lib.svt_amd_md_picture_warmup(ctx, obj.pic))
    obj.blocking()                                                             # first calls: allocations, code objects
    ok(lib, M.launch(lib, ctx, obj.pic, job, inp))
    ok(lib, lib.svt_amd_synchronize(ctx))
    inside = {"blocking": [], "launch": []}
    done = {"blocking": [], "launch": []}
    for _ in range(REPS):
        t0 = time.perf_counter()
        want = obj.blocking()
        done["blocking"].append(time.perf_counter() - t0)                       # (with the three host result arrays allocated and filled around the call: an upper bound)
        inside["blocking"].append(obj.seconds)
        t0 = time.perf_counter()
        rc = M.launch(lib, ctx, obj.pic, job, inp)
        t1 = time.perf_counter()
        ok(lib, rc)
        ok(lib, lib.svt_amd_synchronize(ctx))
        t2 = time.perf_counter()
        inside["launch"].append(t1 - t0), done["launch"].append(t2 - t0)
    same_call(want, M.fetch(lib, ctx, obj.pic, obj.n), tag)
    inp.free()
    obj.free()
    lib.svt_amd_context_destroy(ctx)
    return {"picture": tag, "lcus": obj.n, "inter": obj.inter, "host_ms_inside_the_call": {k_: ms(v) for k_, v in inside.items()},
            "ms_call_to_completed": {"blocking_with_records_on_the_host": ms(inside["blocking"]), "blocking_with_its_host_arrays_allocated_and_filled": ms(done["blocking"]),
                                     "launch_then_synchronize_records_in_hbm": ms(done["launch"])},
            "results_identical": True}


def mode_host(lib):
    out = [host_times(lib, M.load("i_motion_1920x1080_m10"), 0, "i_motion_1920x1080_m10")]
    if os.path.exists(FX_4K):
        out.append(host_times(lib, G(np.load(FX_4K)), 0, "4K B picture 0 of tools/_fx/md4k.npz"))
    else:
        out.append({"picture": "4K B", "skipped": "tools/_fx/md4k.npz is not here"})
    print(json.dumps({"mode": "host", "pictures": out}))


def mode_chain(lib):
    import test_gpu_picture_tail as TT
    from test_gpu_tmvp import load_pair
    name, (q, p) = "motion_416x240_m8", (2, 3)
    gq, gp = load_pair(name)
    w, h = int(gq["pic"][0]["width"]), int(gq["pic"][0]["height"])
    n = S.lcu_count(w, h)
    sg, _, _ = TT.load_case("sao_i_noise_200x136_m6")
    sao, enable = TT.params_of(sg["sao"][0]), np.ones(n, np.uint8)
    ctx = make_context(lib, w, (h + 7) & ~7, 2)
    kq, kp = gq["picture_number"].tolist().index(q), gp["picture_number"].tolist().index(p)
    Q, Pp = M.Obj(lib, ctx, gq, kq), M.Obj(lib, ctx, gp, kp)
    jb, rec, want_ctl = M.device_made_controls(lib, Pp)
    pics, ctl = Pictures(lib, ctx, w, h, [jb], [rec]), Out(lib, ctx, 1, w, h)
    inq, inp = Q.inputs(), Pp.inputs(tmvp=False)
    field, stats = DeviceBuffer(lib, ctx, (n + 1) * FIELD_REC + 256), DeviceBuffer(lib, ctx, 256)
    poc = np.ascontiguousarray(Q.X["ref_poc"][0], np.uint64)
    st = int(Q.P["slice_type"][0])
    tail = TT.Tail(lib, ctx, Q.pic, w, h, False, None, TT.FULL, st, (int(poc[0]), int(poc[1])), sao, enable, (80, 80))
    jq, jp = M.make_job(Q, inq), M.make_job(Pp, inp, d_lcus=ctl.at(), d_tmvp=field.ptr.value)

    def behind_q():
        ok(lib, tail.launch())
        ok(lib, lib.svt_amd_encdec_picture_motion_field(ctx, Q.pic, st, poc.ctypes.data, field.ptr, stats.ptr))
        ok(lib, controls_launch(lib, ctx, pics.job_array([0]), 1, w, h, ctl.at()))

    def launched():
        ok(lib, M.launch(lib, ctx, Q.pic, jq, inq))
        behind_q()
        ok(lib, M.launch(lib, ctx, Pp.pic, jp, inp))
        ok(lib, lib.svt_amd_synchronize(ctx))

    def blocking():
        Q.blocking()
        behind_q()
        ok(lib, lib.svt_amd_md_picture_set_controls(ctx, Pp.pic, C.c_void_p(ctl.at())))
        ok(lib, lib.svt_amd_md_picture_set_motion_field(ctx, Pp.pic, field.ptr))
        s = Pp.src
        out = np.zeros(n, S.MD_LCU_OUT_DTYPE)
        works, res = np.zeros(n, S.LCU_WORK_DTYPE), np.zeros(n, S.LCU_RESULT_DTYPE)
        rc = lib.svt_amd_md_encode_picture_inter(ctx, Pp.pic, Pp.P.ctypes.data, Pp.X.ctypes.data, None, s[0].ctypes.data, s[0].shape[1], s[1].ctypes.data, s[2].ctypes.data,
                                                 s[1].shape[1], Pp.ois.ctypes.data, 0, Pp.me.ctypes.data, 0, None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        ok(lib, rc)
        ok(lib, lib.svt_amd_synchronize(ctx))
        return out.tobytes(), works.tobytes(), res.tobytes()

    ok(lib, lib.svt_amd_synchronize(ctx))
    blocking(), launched()                                                     # first calls
    times = {"blocking": [], "launch": []}
    for _ in range(REPS):
        t0 = time.perf_counter()
        want = blocking()
        times["blocking"].append(time.perf_counter() - t0)                      # (includes allocating the host result arrays of both pictures)
        t0 = time.perf_counter()
        launched()
        times["launch"].append(time.perf_counter() - t0)
    same_call(want, M.fetch(lib, ctx, Pp.pic, n), "chain")
    print(json.dumps({"mode": "chain", "pair": [name, q, p], "lcus": n, "ms_first_call_to_completed_results": {k: ms(v) for k, v in times.items()}, "results_identical": True}))


class Obj16(M.Obj):
    """the same picture with 10-bit samples: source and reference pictures widened as tests/test_gpu_md.py:503 widens them, a 16-bit picture object"""

    def __init__(self, lib, ctx, g, k):
        self.lib, self.ctx, self.g, self.bps = lib, ctx, g, 2
        self.w, self.h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
        self.inter, self.pic, self.keep = True, C.c_void_p(), {}
        ok(lib, lib.svt_amd_encdec_picture_create(ctx, self.w, self.h, 2, C.byref(self.pic)))
        self.load(k)

    def load(self, k):
        import torch
        from test_oracle_md_golden import inter_inputs
        super().load(k)
        rng = np.random.default_rng(11)
        widen = lambda a: ((a.astype(np.uint16) << 2) | rng.integers(0, 4, a.shape, dtype=np.uint16)).astype(np.uint16)  # noqa: E731
        self.src = [widen(a) for a in self.src]
        _, _, _, refs, planes = inter_inputs(self.g, k)
        dev = [[torch.from_numpy(widen(a).view(np.int16)).cuda() for a in pl] for pl in planes]
        torch.cuda.synchronize()
        self.keep[("wide", k)] = dev
        rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r.strideY, r.strideC, r.originX, r.originY, r.width, r.height) for d, r in zip(dev, refs)]
        ok(self.lib, self.lib.svt_amd_encdec_picture_set_inter(self.ctx, self.pic, C.byref(rs[0]), C.byref(rs[1]), self.cost.ctypes.data))

    def blocking(self, lcus=None):
        n, s = self.n, self.src
        out, works, res = np.zeros(n, S.MD_LCU_OUT_DTYPE), np.zeros(n, S.LCU_WORK16_DTYPE), np.zeros(n, S.LCU_RESULT16_DTYPE)
        rc = self.lib.svt_amd_md_encode_picture_inter16(self.ctx, self.pic, self.P.ctypes.data, self.X.ctypes.data, self.lcus.ctypes.data, s[0].ctypes.data, s[0].shape[1],
                                                        s[1].ctypes.data, s[2].ctypes.data, s[1].shape[1], self.ois.ctypes.data, 0, self.me.ctypes.data, 0,
                                                        self.tmvp.ctypes.data if self.tmvp is not None else None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        ok(self.lib, rc)
        return out.tobytes(), works.tobytes(), res.tobytes()


def mode_source(lib):
    """picture 0 of the recorded 4K B pictures at 8 and at 10 bits (source and reference pictures widened)"""
    vp = C.c_void_p
    lib.svt_amd_md_encode_picture_inter16.restype = C.c_int
    lib.svt_amd_md_encode_picture_inter16.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    if not os.path.exists(FX_4K):
        print(json.dumps({"mode": "source", "skipped": "tools/_fx/md4k.npz is not here (tools/md_record_4k.py records it)"}))
        return
    g = G(np.load(FX_4K))
    w, h = int(g["pic"][0]["width"]), int(g["pic"][0]["height"])
    for bps in (1, 2):
        ctx = make_context(lib, w, (h + 7) & ~7, 2)
        obj = (Obj16 if bps == 2 else M.Obj)(lib, ctx, g, 0)
        inp = obj.inputs()
        job = M.make_job(obj, inp, M.tiles_of(obj.lcus))
        for _ in range(3):
            ok(lib, M.launch(lib, ctx, obj.pic, job, inp))
            ok(lib, lib.svt_amd_synchronize(ctx))
            want = obj.blocking()
        ok(lib, M.launch(lib, ctx, obj.pic, job, inp))
        ok(lib, lib.svt_amd_synchronize(ctx))
        same_call(want, M.fetch(lib, ctx, obj.pic, obj.n, bps == 2), bps)
        moved = sum(a.nbytes for a in obj.src)
        print(json.dumps({"mode": "source", "bytes_per_sample": bps, "width": w, "height": h, "plane_bytes_read": moved,
                          "plane_bytes_written": moved + (moved // 2 if bps == 2 else 0), "results_identical": True}))
        inp.free()
        obj.free()
        lib.svt_amd_context_destroy(ctx)


if __name__ == "__main__":
    {"host": mode_host, "chain": mode_chain, "source": mode_source}[sys.argv[1]](library())
