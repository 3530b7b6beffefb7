"""ctypes views and prototypes of the stream-ordered mode-decision launch (include/svt_hevc_amd.h "Device-resident mode decision":
svt_amd_md_encode_picture_launch, svt_amd_encdec_picture_md_records); tests/test_mdlaunch_abi.py holds them against the header.  DeviceInputs: every input of one picture's
launch in device memory; Obj: a picture object that shares a lane with others (the GPU tests and tools/md_launch_time.py)."""
import ctypes as C
import os
import time

import numpy as np

import mdctl_numpy as N
import mdctl_records as R
import svtlib as S
from pa_batch_util import SENTINEL, ok
from test_oracle_md_golden import inter_inputs

ENTRY = "svt_amd_md_encode_picture_launch"
RECORDS_ENTRY = "svt_amd_encdec_picture_md_records"
DECIDE_ONLY = 1                    # SVT_AMD_MD_LAUNCH_DECIDE_ONLY
u32, i32, vp = C.c_uint32, C.c_int32, C.c_void_p


class CtlCheck(C.Structure):
    _fields_ = [("bad_leaf_count", u32), ("bad_leaf_list", u32), ("md_mode", u32 * 16), ("bad_chroma", u32), ("tiles", u32), ("first_bad", u32), ("first_kind", u32)]


class LaunchJob(C.Structure):
    _fields_ = [("P", vp), ("X", vp), ("cost", vp), ("d_lcus", vp), ("d_src", vp * 3), ("d_ois", vp), ("d_me", vp), ("d_tmvp", vp), ("src_pitch_y", u32),
                ("src_pitch_c", u32), ("ois_slot", i32), ("me_slot", i32), ("tiles", u32), ("flags", u32), ("pad", u32 * 2)]


class LaunchStatus(C.Structure):
    _fields_ = [("check", CtlCheck), ("refused", u32), ("pad", u32)]


assert C.sizeof(LaunchJob) == 112 and C.sizeof(LaunchStatus) == 96 and C.sizeof(CtlCheck) == 88


def declare(lib):
    lib.svt_amd_md_encode_picture_launch.restype, lib.svt_amd_md_encode_picture_launch.argtypes = C.c_int, [vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_md_records.restype, lib.svt_amd_encdec_picture_md_records.argtypes = C.c_int, [vp] * 6
    lib.svt_amd_md_picture_set_controls.restype, lib.svt_amd_md_picture_set_controls.argtypes = C.c_int, [vp, vp, vp]
    lib.svt_amd_md_picture_set_motion_field.restype, lib.svt_amd_md_picture_set_motion_field.argtypes = C.c_int, [vp, vp, vp]
    lib.svt_amd_md_picture_supported.restype, lib.svt_amd_md_picture_supported.argtypes = C.c_int, [vp]
    lib.svt_amd_md_picture_warmup.restype, lib.svt_amd_md_picture_warmup.argtypes = C.c_int, [vp, vp]
    lib.svt_amd_synchronize.restype, lib.svt_amd_synchronize.argtypes = C.c_int, [vp]
    lib.svt_amd_debug_md_kernel_ms.restype, lib.svt_amd_debug_md_kernel_ms.argtypes = C.c_int, [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib


def kernel_width(lib, ctx, pic):
    """the workgroups of the picture object's last mode-decision kernel, blocking call or launch (svt_amd_debug_md_kernel_ms waits for that kernel)"""
    ms, workgroups = C.c_float(), C.c_int(-1)
    ok(lib, lib.svt_amd_debug_md_kernel_ms(ctx, pic, C.byref(ms), C.byref(workgroups)))
    return workgroups.value


def up(n):
    return (n + 255) & ~255


def record_arrays(lib, pic):
    """(d_out, d_works, work stride, d_results, result stride) of the picture object"""
    out, works, res, ws, rs = vp(), vp(), vp(), C.c_size_t(), C.c_size_t()
    rc = lib.svt_amd_encdec_picture_md_records(pic, C.byref(out), C.byref(works), C.byref(ws), C.byref(res), C.byref(rs))
    assert rc == 0, lib.svt_amd_last_error()
    return out.value, works.value, ws.value, res.value, rs.value


class DeviceInputs:
    """the device inputs of one picture's launch in ONE allocation filled with the sentinel: controls, source planes at `extra` samples of pitch beyond the width and
    `base` bytes behind a 256-byte boundary, OIS / ME records, the motion field with its zero record behind the last LCU, and the status record with a guard"""
    GUARD = 256

    def __init__(self, lib, ctx, lcus, src, ois, me=None, tmvp=None, extra=0, base=0):
        from pa_batch_util import DeviceBuffer, ok
        self.lib, self.ctx = lib, ctx
        planes = []
        for a in src:
            p = np.zeros((a.shape[0], a.shape[1] + extra), a.dtype)
            p[:, :a.shape[1]] = a
            p[:, a.shape[1]:] = 0x5A                                    # what a launch that read the padding would see
            planes.append(p)
        parts = [("lcus", np.ascontiguousarray(lcus), 0)] + [("src%d" % k, p, base) for k, p in enumerate(planes)] + [("ois", np.ascontiguousarray(ois), 0)]
        if me is not None:
            parts.append(("me", np.ascontiguousarray(me), 0))
        if tmvp is not None:
            field = np.zeros(len(tmvp) + 1, tmvp.dtype)
            field[:len(tmvp)] = tmvp
            parts.append(("tmvp", field, 0))
        self.at, self.keep, off = {}, {}, 0
        for name, a, b in parts:
            self.at[name], self.keep[name] = off + b, a
            off += up(b + a.nbytes)
        self.at["status"] = off
        self.dev = DeviceBuffer(lib, ctx, off + C.sizeof(LaunchStatus) + self.GUARD)
        for name, a, b in parts:                                        # blocking uploads: nothing of the inputs is in flight when a test starts its sequence
            ok(lib, lib.svt_amd_device_upload(ctx, vp(self.dev.at(self.at[name])), a.ctypes.data, a.nbytes))
        self.pitch = (planes[0].shape[1], planes[1].shape[1])

    def ptr(self, name):
        return self.dev.at(self.at[name]) if name in self.at else None

    def status(self, raw=None):
        """the status record, downloaded; the bytes behind it must be untouched"""
        from pa_batch_util import is_sentinel
        raw = self.dev.get() if raw is None else raw
        at = self.at["status"]
        assert is_sentinel(raw[at + C.sizeof(LaunchStatus):]), "bytes behind the status record"
        return LaunchStatus.from_buffer_copy(raw[at:at + C.sizeof(LaunchStatus)].tobytes())

    def inputs_unchanged(self, raw=None):
        raw = self.dev.get() if raw is None else raw
        for name, a in self.keep.items():
            at = self.at[name]
            if raw[at:at + a.nbytes].tobytes() != a.tobytes():
                return False
        return True

    def free(self):
        self.dev.free()


def make_job(world, inputs, tiles=1, flags=0, d_lcus=None, d_tmvp=None, cost=True):
    """the job of `world`'s picture (an MdWorld of tests/test_gpu_mdctl_batch.py, or anything with P, X, cost, inter) from `inputs`"""
    j = LaunchJob()
    j.P = world.P.ctypes.data
    j.X = world.X.ctypes.data if world.inter else None
    j.cost = world.cost.ctypes.data if cost else None
    j.d_lcus = inputs.ptr("lcus") if d_lcus is None else d_lcus
    for k in range(3):
        j.d_src[k] = inputs.ptr("src%d" % k)
    j.src_pitch_y, j.src_pitch_c = inputs.pitch
    j.d_ois, j.d_me = inputs.ptr("ois"), inputs.ptr("me")
    j.d_tmvp = inputs.ptr("tmvp") if d_tmvp is None else d_tmvp
    j.ois_slot, j.me_slot, j.tiles, j.flags = -1, -1, tiles, flags
    return j


def launch(lib, ctx, pic, job, inputs=None):
    return lib.svt_amd_md_encode_picture_launch(ctx, pic, C.byref(job), vp(inputs.ptr("status")) if inputs is not None else None)


def fetch(lib, ctx, pic, n, wide=False):
    """the object's three arrays as bytes (blocking downloads on the context's lane)"""
    d_out, d_works, ws, d_res, rs = record_arrays(lib, pic)
    assert ws == (S.LCU_WORK16_DTYPE if wide else S.LCU_WORK_DTYPE).itemsize and rs == (S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE).itemsize
    got = []
    for ptr, size in ((d_out, S.MD_LCU_OUT_DTYPE.itemsize), (d_works, ws), (d_res, rs)):
        a = np.zeros(n * size, np.uint8)
        rc = lib.svt_amd_device_download(ctx, a.ctypes.data, vp(ptr), a.nbytes)
        assert rc == 0, lib.svt_amd_last_error()
        got.append(a.tobytes())
    return tuple(got)


def load(name):
    return np.load(os.path.join(S.GOLDEN_DIR, "md_%s.npz" % name))


def tiles_of(lcus):
    return int(((lcus["tile_left"] != 0) & (lcus["tile_top"] != 0)).sum())


class Obj:
    """a picture object on `ctx` that takes picture k of a fixture (load: inputs, reference pictures); blocking() -> the blocking call's three arrays.
    preload(k): picture k's reference pictures into device memory (this waits); load(k) of a preloaded picture waits for nothing"""

    def __init__(self, lib, ctx, g, k):
        self.lib, self.ctx, self.g, self.bps = lib, ctx, g, 1
        self.w, self.h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
        self.inter = "inter" in g.files
        self.pic, self.keep = vp(), {}
        ok(lib, lib.svt_amd_encdec_picture_create(ctx, self.w, self.h, 1, C.byref(self.pic)))
        self.load(k)

    def preload(self, k):
        import torch
        if self.inter and k not in self.keep:                                   # reference pictures of every picture loaded stay: launches may be in flight
            _, _, _, refs, planes = inter_inputs(self.g, k)
            dev = [[torch.from_numpy(a).cuda() for a in pl] for pl in planes]
            torch.cuda.synchronize()
            self.keep[k] = (dev, [(r.strideY, r.strideC, r.originX, r.originY, r.width, r.height) for r in refs])

    def load(self, k):
        g, lib = self.g, self.lib
        self.preload(k)
        self.k = k
        self.P = np.ascontiguousarray(g["pic"][k:k + 1])
        self.cost, self.ois = np.ascontiguousarray(g["cost"][k]), np.ascontiguousarray(g["ois"][k])
        self.src = [np.ascontiguousarray(g[n][k]) for n in ("src_y", "src_cb", "src_cr")]
        self.lcus = np.ascontiguousarray(g["lcu"][k])
        self.n = len(self.lcus)
        self.X = self.me = self.tmvp = None
        if self.inter:
            self.X, self.me, self.tmvp, _, _ = inter_inputs(g, k)
            dev, geom = self.keep[k]
            rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), *r) for d, r in zip(dev, geom)]
            ok(lib, lib.svt_amd_encdec_picture_set_inter(self.ctx, self.pic, C.byref(rs[0]), C.byref(rs[1]), self.cost.ctypes.data))

    def inputs(self, tmvp=True, **kw):
        return DeviceInputs(self.lib, self.ctx, self.lcus, self.src, self.ois, self.me, self.tmvp if tmvp else None, **kw)

    def blocking(self, lcus=None):
        lib, n, s = self.lib, self.n, self.src
        lcus = self.lcus if lcus is None else np.ascontiguousarray(lcus)
        out = np.full(n * S.MD_LCU_OUT_DTYPE.itemsize, SENTINEL, np.uint8)
        works = np.full(n * S.LCU_WORK_DTYPE.itemsize, SENTINEL, np.uint8)
        res = np.full(n * S.LCU_RESULT_DTYPE.itemsize, SENTINEL, np.uint8)
        t0 = time.perf_counter()
        if self.inter:
            rc = lib.svt_amd_md_encode_picture_inter(self.ctx, self.pic, self.P.ctypes.data, self.X.ctypes.data, lcus.ctypes.data, s[0].ctypes.data, s[0].shape[1],
                                                     s[1].ctypes.data, s[2].ctypes.data, s[1].shape[1], self.ois.ctypes.data, 0, self.me.ctypes.data, 0,
                                                     self.tmvp.ctypes.data if self.tmvp is not None else None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        else:
            rc = lib.svt_amd_md_encode_picture(self.ctx, self.pic, self.P.ctypes.data, lcus.ctypes.data, s[0].ctypes.data, s[0].shape[1], s[1].ctypes.data,
                                               s[2].ctypes.data, s[1].shape[1], self.ois.ctypes.data, 0, self.cost.ctypes.data, out.ctypes.data, works.ctypes.data,
                                               res.ctypes.data)
        self.seconds = time.perf_counter() - t0                                # host time inside the blocking call alone
        assert rc == 0, lib.svt_amd_last_error()
        return out.tobytes(), works.tobytes(), res.tobytes()

    def free(self):
        self.lib.svt_amd_encdec_picture_destroy(self.ctx, self.pic)


def device_made_controls(lib, obj):
    """inputs of svt_amd_md_controls_batch_launch whose controls the P / B call covers: seeded records (tests/mdctl_records.py) under the fixture's own leaf lists and
    LCU modes -> (job scalars, records, the controls the restatement expects)"""
    depth, level = int(obj.P["depth_mode"][0]), int(obj.P["chroma_level"][0])
    jb = R.job(R.B, depth, level, 0, tiles=(1, 1))
    for seed in range(101, 121):
        rec = R.make_inputs(obj.w, obj.h, seed, 0, jb)
        for f in ("leaf_count", "leaf_index", "leaf_split", "lcu_md_mode"):
            rec["mdc_lcu"][f] = obj.lcus[f]
        want = np.ascontiguousarray(N.md_controls(obj.w, obj.h, rec, jb))
        if lib.svt_amd_md_lcus_supported(obj.P.ctypes.data, want.ctypes.data, len(want)) == 1:
            return jb, rec, want
    raise AssertionError("no seed gives controls the call covers")
