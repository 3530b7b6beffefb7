"""GPU: the mode-decision picture call as a stream-ordered launch on device inputs (include/svt_hevc_amd.h: svt_amd_md_encode_picture_launch,
svt_amd_encdec_picture_md_records; svt-hevc_amd/csrc/mdlaunch_kernels.hip and the entry in md_picture.hip) - against the blocking call on the same picture object,
byte for byte, and against the decisions the REFERENCE recorded (tests/golden/md_*.npz); source planes at awkward pitches; launches in flight on one lane; the chain
controls -> decision -> tail -> motion field -> next decision without a wait; a controls array refused on the device; the host time of the call."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import mdctl_numpy as N
import mdlaunchlib as M
import svtlib as S
import taillib
import tmvplib as T
from pa_batch_util import BAD_PARAM, SENTINEL, DeviceBuffer, is_sentinel, make_context, ok, refused
from test_gpu_mdctl_batch import MdWorld, Out, Pictures, Rect, _md_sig, decisions, launch as controls_launch, same_call
from mdlaunchlib import Obj, device_made_controls, load, tiles_of
from test_oracle_md_golden import compare_md, inter_inputs

pytestmark = pytest.mark.gpu
vp = C.c_void_p
GUARD = 256
FIELD_REC = T.TMVP_LCU_DTYPE.itemsize
RESULTS = {}                           # (fixture, bytes per sample, k) -> the launch's three arrays of case 1, shared with case 2


@pytest.fixture(scope="module")
def lib(product):
    _md_sig(product)
    vp_ = C.c_void_p
    product.svt_amd_md_encode_picture_inter16.restype = C.c_int
    product.svt_amd_md_encode_picture_inter16.argtypes = [vp_, vp_, vp_, vp_, vp_, vp_, C.c_uint32, vp_, vp_, C.c_uint32, vp_, C.c_int, vp_, C.c_int, vp_, vp_, vp_, vp_]
    product.svt_amd_encdec_picture_set_rect.restype, product.svt_amd_encdec_picture_set_rect.argtypes = C.c_int, [vp_, vp_, vp_]
    return taillib.declare(T.declare(M.declare(product)))


class World(MdWorld):
    """MdWorld, and the 10-bit P / B picture it does not set up: 16-bit reference pictures (the fixture's widened, tests/test_gpu_md.py:503) and the blocking call
    through svt_amd_md_encode_picture_inter16"""

    def __init__(self, lib, g, k=0, bps=1):
        import torch
        super().__init__(lib, g, k, bps)
        if bps == 2 and self.inter:
            rng = np.random.default_rng(11)
            _, _, _, refs, planes = inter_inputs(g, k)
            wide = [[((a.astype(np.uint16) << 2) | rng.integers(0, 4, a.shape, dtype=np.uint16)).astype(np.uint16) for a in pl] for pl in planes]
            self.ref_dev = [[torch.from_numpy(a.view(np.int16)).cuda() for a in pl] for pl in wide]
            torch.cuda.synchronize()
            rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r.strideY, r.strideC, r.originX, r.originY, r.width, r.height)
                  for d, r in zip(self.ref_dev, refs)]
            ok(lib, lib.svt_amd_encdec_picture_set_inter(self.ctx, self.pic, C.byref(rs[0]), C.byref(rs[1]), self.cost.ctypes.data))

    def call(self, host=None, **kw):
        if not (self.bps == 2 and self.inter):
            return super().call(host=host, **kw)
        n, s = self.n, self.src
        out = np.full(n, SENTINEL, np.uint8).repeat(S.MD_LCU_OUT_DTYPE.itemsize).view(S.MD_LCU_OUT_DTYPE)
        works = np.full(n * S.LCU_WORK16_DTYPE.itemsize, SENTINEL, np.uint8)
        res = np.full(n * S.LCU_RESULT16_DTYPE.itemsize, SENTINEL, np.uint8)
        hp = np.ascontiguousarray(host)
        rc = self.lib.svt_amd_md_encode_picture_inter16(self.ctx, self.pic, self.P.ctypes.data, self.X.ctypes.data, hp.ctypes.data, s[0].ctypes.data, s[0].shape[1],
                                                        s[1].ctypes.data, s[2].ctypes.data, s[1].shape[1], self.ois.ctypes.data, 0, self.me.ctypes.data, 0,
                                                        self.tmvp.ctypes.data if self.tmvp is not None else None, out.ctypes.data, works.ctypes.data, res.ctypes.data)
        return rc, (out.tobytes(), works.tobytes(), res.tobytes())

    def inputs(self, lcus=None, **kw):
        return M.DeviceInputs(self.lib, self.ctx, self.lcus if lcus is None else lcus, self.src, self.ois, self.me if self.inter else None,
                              self.tmvp if self.inter else None, **kw)


def launched(lib, world, inp, want_refused=0, lcus=None):
    """one launch, one synchronise, the three arrays; the status record is the restatement's summary, nothing behind it is written, no input has changed"""
    lcus = world.lcus if lcus is None else lcus
    ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, tiles_of(lcus)), inp))
    ok(lib, lib.svt_amd_synchronize(world.ctx))
    got = M.fetch(lib, world.ctx, world.pic, world.n, world.bps == 2)
    raw = inp.dev.get()
    st = inp.status(raw)
    assert inp.inputs_unchanged(raw)
    depth = int(world.P["depth_mode"][0])
    assert bytes(st.check) == N.check_summary(lcus, depth, world.inter).tobytes() and st.refused == want_refused and st.pad == 0
    return got, st


# ---- 1. the launch equals the blocking call and the reference ------------------------------------------------------------------------------------------

FIXTURES = [("i_xc_binary_192x128_m9_q0", 1), ("i_motion_416x240_m9", 1), ("i_motion_416x240_m9", 2), ("b_xc_whiteblack_192x128_m8_q0", 1),
            ("b_xc_binary_200x136_m8_q51", 1), ("bref_xc_whiteblack_192x128_m8_q0", 1), ("p_objects_320x192_m8_ld", 1), ("b_tiles_motion_640x384_m8", 1),
            ("b_motion_416x240_m8", 2)]                                       # the order of the issue's table


def case_one(lib, name, bps, k):
    """the launch's three arrays for picture k of a fixture at the plain pitch, checked against the blocking call and the reference; computed once"""
    if (name, bps, k) not in RESULTS:
        g = load(name)
        world = World(lib, g, k, bps)
        inp = world.inputs()
        try:
            got, st = launched(lib, world, inp)
            assert st.check.first_bad == 0xFFFFFFFF
            rc, want = world.call(host=world.lcus)
            assert rc == 0, lib.svt_amd_last_error()
            same_call(want, got, (name, bps, k))
            compare_md(np.frombuffer(got[0], S.MD_LCU_OUT_DTYPE), g["out"][k], "%s picture %d, %d bytes a sample" % (name, k, bps))
            RESULTS[(name, bps, k)] = got
        finally:
            inp.free()
            world.free()
    return RESULTS[(name, bps, k)]


@pytest.mark.parametrize("name,bps", FIXTURES)
def test_launch_equals_the_blocking_call_and_the_reference(lib, name, bps):
    """every input uploaded, the launch, ONE synchronise, the arrays through svt_amd_encdec_picture_md_records: the blocking call's bytes on the same object (the
    launch runs first, on a fresh object: nothing of a blocking call can be left in the arrays), and the reference's own decisions"""
    g = load(name)
    if name.startswith("b_tiles"):
        assert tiles_of(g["lcu"][0]) == 4
    if name.startswith("bref_xc"):
        assert (g["lcu"][:2]["chroma_encode_mode"] == 1).any()                # CHROMA_MODE_FULL LCUs (picture 1)
    for k in range(min(2, len(g["picture_number"]))):
        case_one(lib, name, bps, k)


# ---- 1b. both entries take one launch width ----------------------------------------------------------------------------------------------------------------

WIDTH_OVERRIDES = ("SVT_AMD_MD_GRID", "SVT_AMD_MD_NARROW", "SVT_AMD_MD_WIDE", "SVT_AMD_MD_MAX_KERNELS", "SVT_AMD_MD_WG_BUDGET")


@pytest.mark.parametrize("name,bps,lone", [("i_xc_binary_192x128_m9_q0", 1, 6), ("b_motion_416x240_m8", 1, 10), ("b_motion_416x240_m8", 2, 10),
                                           ("b_tiles_motion_640x384_m8", 1, 42)])
def test_both_entries_take_the_same_width_on_an_idle_device(lib, name, bps, lone):
    """no result depends on the launch width, so case 1 cannot see an entry that computes its own: the blocking call on a fresh object, then a launch on the same
    object, each with nothing else on the device - svt_amd_debug_md_kernel_ms reports the `lone` width tests/test_md_widths_cpu.py pins for the shape (the arm that
    the LCU count clamps, the plain one, four tiles)"""
    overridden = [v for v in WIDTH_OVERRIDES if v in os.environ]
    if overridden:
        pytest.skip("%s set: the launch widths are overridden for a measurement" % ", ".join(overridden))
    g = load(name)
    world = World(lib, g, 0, bps)
    inp = world.inputs()
    try:
        rc, _ = world.call(host=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()
        assert M.kernel_width(lib, world.ctx, world.pic) == lone
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, tiles_of(world.lcus)), inp))
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        assert inp.status().refused == 0
        assert M.kernel_width(lib, world.ctx, world.pic) == lone
    finally:
        inp.free()
        world.free()


# ---- 2. source planes at awkward pitches and alignments ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bps", [("i_xc_binary_192x128_m9_q0", 1), ("b_xc_binary_200x136_m8_q51", 1), ("i_motion_416x240_m9", 2)])
def test_source_planes_at_pitch_plus_four_and_a_base_offset_of_four_bytes(lib, name, bps):
    """rows that start 16-byte aligned and rows that do not, in one plane (the copy's two paths); the pad columns hold 0x5A, which no result may depend on"""
    g = load(name)
    world = World(lib, g, 0, bps)
    inp = world.inputs(extra=4, base=4)
    try:
        assert inp.pitch == (world.w + 4, world.w // 2 + 4) and inp.ptr("src0") % 16 == 4
        got, _ = launched(lib, world, inp)
        rc, want = world.call(host=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()
        same_call(want, got, name)
        first = case_one(lib, name, bps, 0)                                    # the same bytes as case 1 (another object: the never-written pad of md_out may differ)
        assert got[1] == first[1] and got[2] == first[2], name
    finally:
        inp.free()
        world.free()


# ---- 3. two launches in flight do not share staging ---------------------------------------------------------------------------------------------------

def test_launches_in_flight_on_one_lane_keep_their_own_inputs(lib):
    """behind an I picture that keeps the lane busy, pictures 0 and 1 of a fixture (another QP, picture number and rate tables) into two objects, then both into a
    THIRD object, back to back, with nothing between the launches that waits: every reference picture is on the device before the sequence starts, and between
    the two launches into the shared object lie only svt_amd_encdec_picture_set_inter (host state and one asynchronous copy) and three asynchronous downloads into
    page-locked memory - the shared object's arrays as its FIRST launch leaves them, which the second then overwrites.  A launch's small inputs are captured when it
    is queued: the snapshot holds picture 0's results and every object ends up with the results of the picture launched into it last.  Staged through one host block
    per object (the blocking call's h_stage), the shared object's first launch would read the second one's P, X and rate tables and the snapshot would differ;
    staged through one block per lane, the first two objects would too"""
    gi, g = load("i_motion_416x240_m9"), load("bref_motion_416x240_m8")
    assert [int(g["pic"][k]["qp"]) for k in (0, 1)] == [35, 33] and g["inter"][0]["picture_number"] != g["inter"][1]["picture_number"]
    assert g["cost"][0].tobytes() != g["cost"][1].tobytes()
    lib.svt_amd_host_alloc.restype, lib.svt_amd_host_alloc.argtypes = C.c_int, [vp, C.c_size_t, C.POINTER(vp)]
    lib.svt_amd_host_free.restype, lib.svt_amd_host_free.argtypes = C.c_int, [vp, vp]
    lib.svt_amd_device_download_async.restype, lib.svt_amd_device_download_async.argtypes = C.c_int, [vp, vp, vp, C.c_size_t]
    ctx = make_context(lib, 416, 240, 2)
    busy, a, b, c = Obj(lib, ctx, gi, 0), Obj(lib, ctx, g, 0), Obj(lib, ctx, g, 1), Obj(lib, ctx, g, 0)
    c.preload(1)                                                                # picture 1's reference pictures: on the device now, so that load(1) below waits for nothing
    ins = [busy.inputs(), a.inputs(), b.inputs()]
    sizes = (S.MD_LCU_OUT_DTYPE.itemsize * c.n, S.LCU_WORK_DTYPE.itemsize * c.n, S.LCU_RESULT_DTYPE.itemsize * c.n)
    pinned = [vp() for _ in sizes]
    try:
        for h, size in zip(pinned, sizes):
            ok(lib, lib.svt_amd_host_alloc(ctx, size, C.byref(h)))
        ok(lib, lib.svt_amd_md_picture_warmup(ctx, c.pic))
        d_out, d_works, _, d_res, _ = M.record_arrays(lib, c.pic)
        jobs = [M.make_job(o, i) for o, i in zip((busy, a, b), ins)]
        ok(lib, lib.svt_amd_synchronize(ctx))
        ok(lib, M.launch(lib, ctx, busy.pic, jobs[0]))
        ok(lib, M.launch(lib, ctx, a.pic, jobs[1]))
        ok(lib, M.launch(lib, ctx, b.pic, jobs[2]))
        ok(lib, M.launch(lib, ctx, c.pic, jobs[1]))                             # picture 0 into the shared object ...
        for h, d, size in zip(pinned, (d_out, d_works, d_res), sizes):          # ... what it leaves, queued behind it ...
            ok(lib, lib.svt_amd_device_download_async(ctx, h, vp(d), size))
        c.load(1)                                                               # (host state of the object, read at queue time; no wait: preloaded)
        ok(lib, M.launch(lib, ctx, c.pic, M.make_job(c, ins[2])))               # ... and picture 1 behind it, before anything has run to its end
        ok(lib, lib.svt_amd_synchronize(ctx))
        first = tuple(C.string_at(h, size) for h, size in zip(pinned, sizes))
        got = {o: M.fetch(lib, ctx, o.pic, o.n) for o in (a, b, c)}
        want = {o: o.blocking() for o in (a, b, c)}
        for tag, o in (("picture 0 in its own object", a), ("picture 1 in its own object", b), ("picture 1 launched last into the shared object", c)):
            same_call(want[o], got[o], tag)
        c.load(0)
        same_call(c.blocking(), first, "picture 0 as the shared object's first launch left it")
        assert got[a][1] != got[b][1] and got[c][1] == got[b][1] and first[1] == got[a][1]
    finally:
        for h in pinned:
            if h:
                lib.svt_amd_host_free(ctx, h)
        for i in ins:
            i.free()
        for o in (busy, a, b, c):
            o.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 4. the chain stays on the device -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["motion_416x240_m8", "noise_320x256_m9_q24", "objects_640x360_m9_q36", "xc_binary_200x136_m8_q51"])
def test_the_chain_stays_on_the_device(lib, name):
    """q launched, its tail (all four stages, NULL records) and its motion field queued behind it, p's controls made by svt_amd_md_controls_batch_launch, p launched
    with that field and those controls: one lane, ONE synchronise at the end.  p's arrays equal the blocking call with the recorded host field; q's padded
    reference and SAO parameters equal those of the tail behind q's blocking call"""
    import test_gpu_picture_tail as TT
    from test_gpu_tmvp import load_pair, pair_is_live
    gq, gp = load_pair(name)
    w, h = int(gq["pic"][0]["width"]), int(gq["pic"][0]["height"])
    n = S.lcu_count(w, h)
    sg, _, _ = TT.load_case("sao_i_noise_200x136_m6")
    sao = TT.params_of(sg["sao"][0])
    enable = np.ones(n, np.uint8)
    ctx = make_context(lib, w, (h + 7) & ~7, 2)
    live = []
    try:
        for q, p in dict(T.MD_PAIRS)[name]:
            tag = (name, q, p)
            kq, kp = gq["picture_number"].tolist().index(q), gp["picture_number"].tolist().index(p)
            Q, Pp = Obj(lib, ctx, gq, kq), Obj(lib, ctx, gp, kp)
            assert int(Pp.X["colocated_poc"][0]) == q and Pp.tmvp is not None, tag
            jb, rec, want_ctl = device_made_controls(lib, Pp)
            pics, ctl = Pictures(lib, ctx, w, h, [jb], [rec]), Out(lib, ctx, 1, w, h)
            inq, inp = Q.inputs(), Pp.inputs(tmvp=False)
            field, stats = DeviceBuffer(lib, ctx, (n + 1) * FIELD_REC + GUARD), DeviceBuffer(lib, ctx, GUARD)
            poc = np.ascontiguousarray(Q.X["ref_poc"][0], np.uint64)
            slice_type = int(Q.P["slice_type"][0])
            tails = [TT.Tail(lib, ctx, Q.pic, w, h, False, None, TT.FULL, slice_type, (int(poc[0]), int(poc[1])), sao, enable, (80, 80)) for _ in range(2)]
            try:
                ok(lib, lib.svt_amd_synchronize(ctx))
                ok(lib, M.launch(lib, ctx, Q.pic, M.make_job(Q, inq), inq))
                ok(lib, tails[0].launch())
                ok(lib, lib.svt_amd_encdec_picture_motion_field(ctx, Q.pic, slice_type, poc.ctypes.data, field.ptr, stats.ptr))
                ok(lib, controls_launch(lib, ctx, pics.job_array([0]), 1, w, h, ctl.at()))
                ok(lib, M.launch(lib, ctx, Pp.pic, M.make_job(Pp, inp, d_lcus=ctl.at(), d_tmvp=field.ptr.value), inp))
                ok(lib, lib.svt_amd_synchronize(ctx))                           # the one wait
                got_p = M.fetch(lib, ctx, Pp.pic, n)
                got_pad, got_dec = tails[0].padded(), tails[0].params().copy()
                assert inq.status().refused == 0 and inp.status().refused == 0
                made = ctl.download()[0]
                assert made.tobytes() == want_ctl.tobytes(), tag
                same_call(Pp.blocking(lcus=made), got_p, tag)                  # the recorded host field, the same controls as host records
                Q.blocking()
                ok(lib, tails[1].launch())
                want_pad, want_dec = tails[1].padded(), tails[1].params()
                for k in range(3):
                    assert np.array_equal(got_pad[k], want_pad[k]), (tag, k)
                assert got_dec.tobytes() == want_dec.tobytes(), tag
                if pair_is_live(gp, kp):
                    live.append(tag)
            finally:
                for t in tails:
                    t.free()
                for o in (pics, ctl, inq, inp, field, stats, Q, Pp):
                    o.free()
        if name == "motion_416x240_m8":
            assert live, "no pair with the temporal candidate on and available units in its field"
    finally:
        lib.svt_amd_context_destroy(ctx)


# ---- 5. refused on the device, nothing run ------------------------------------------------------------------------------------------------------------------

def test_a_controls_array_the_host_loop_refuses_decides_and_encodes_nothing(lib):
    """lcu_md_mode 3 in ONE LCU of a B picture under depth mode 0 (its leaf list stays valid: a gate that let the kernels run would show as a failed assertion):
    the status names the LCU, md_out keeps its sentinel, work and result records are zero, the tail counts every LCU whose zero record is not at its raster position
    (all but LCU 0); the same object then takes the good records"""
    import test_gpu_picture_tail as TT
    name = "b_xc_whiteblack_192x128_m8_q0"
    g = load(name)
    world = World(lib, g, 0, 1)
    assert int(world.P["depth_mode"][0]) == 0
    bad = world.lcus.copy()
    bad["lcu_md_mode"][2] = 3
    inp_bad, inp = world.inputs(lcus=bad), world.inputs()
    sg, _, _ = TT.load_case("sao_i_noise_200x136_m6")
    tail = TT.Tail(lib, world.ctx, world.pic, world.w, world.h, False, None, TT.FULL, int(world.P["slice_type"][0]), (1, 3), TT.params_of(sg["sao"][0]),
                   np.ones(world.n, np.uint8), (80, 80))
    try:
        ok(lib, lib.svt_amd_md_picture_warmup(world.ctx, world.pic))            # the object's arrays exist: md_out takes the sentinel
        d_out = M.record_arrays(lib, world.pic)[0]
        poison = np.full(world.n * S.MD_LCU_OUT_DTYPE.itemsize, SENTINEL, np.uint8)
        ok(lib, lib.svt_amd_device_upload(world.ctx, vp(d_out), poison.ctypes.data, poison.nbytes))
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp_bad), inp_bad))
        ok(lib, tail.launch())
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        st = inp_bad.status()
        assert bytes(st.check) == N.check_summary(bad, 0, True).tobytes()
        assert (st.refused, st.check.first_bad, st.check.first_kind, st.pad) == (1, 2, 2, 0)
        out, works, res = M.fetch(lib, world.ctx, world.pic, world.n)
        assert is_sentinel(np.frombuffer(out, np.uint8)) and not any(works) and not any(res)
        chk = tail.check()                                                      # a zero record is LCU (0, 0) without units: LCU 0's is well formed, every other
        assert (int(chk["bad_lcus"]), int(chk["first_bad_lcu"]), int(chk["bad_units"])) == (world.n - 1, 1, 0)    # LCU is not at its raster position
        got, st = launched(lib, world, inp)                                     # the same object, the good records
        rc, want = world.call(host=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()
        same_call(want, got, "after the refusal")
        compare_md(np.frombuffer(got[0], S.MD_LCU_OUT_DTYPE), g["out"][0], name)
    finally:
        tail.free()
        inp_bad.free()
        inp.free()
        world.free()


def test_host_side_refusals_that_need_a_device(lib):
    """the rules tests/test_mdlaunch_abi.py cannot reach without a picture object: tiles, reference pictures, rate tables (P / B and I), row starts at both sample
    widths, the motion field, slot records, a rank rectangle; then DECIDE_ONLY and cost == NULL on an object that has its tables.  Each names the entry; afterwards the launch still gives the blocking call's bytes"""
    g = load("b_motion_416x240_m8")
    world = World(lib, g, 0, 1)
    inp = world.inputs()
    gi = load("i_motion_416x240_m9")
    Pi = np.ascontiguousarray(gi["pic"][0:1])                                  # an I picture of the same size: the rules that need no inter controls
    assert (int(Pi["width"][0]), int(Pi["height"][0])) == (world.w, world.h) and int(world.X["tmvp_enable"][0]) == 1
    bare, bare16 = vp(), vp()                                                   # objects without reference pictures and rate tables, 8 and 16 bits a sample
    ok(lib, lib.svt_amd_encdec_picture_create(world.ctx, world.w, world.h, 1, C.byref(bare)))
    ok(lib, lib.svt_amd_encdec_picture_create(world.ctx, world.w, world.h, 2, C.byref(bare16)))
    try:
        def bad(what, text, pic=None, whole=False, **change):
            j = M.make_job(world, inp, **{k: v for k, v in change.items() if k in ("flags", "cost", "tiles")})
            for f, v in change.items():
                if f not in ("flags", "cost", "tiles"):
                    setattr(j, f, v)
            refused(lib, M.launch(lib, world.ctx, pic or world.pic, j, inp), M.ENTRY, what)
            err = lib.svt_amd_last_error()
            assert err == text if whole else text in err, (what, err)
        bad("tiles 0", b"tiles", tiles=0)
        bad("more tiles than LCUs", b"tiles", tiles=world.n + 1)
        bad("no reference pictures", b"reference pictures / rate tables", pic=bare)
        bad("a P / B picture without rate tables anywhere", b"reference pictures / rate tables", pic=bare, cost=False)
        bad("an I picture without rate tables anywhere", b"no rate tables", pic=bare, cost=False, P=Pi.ctypes.data, X=None)
        # rows have to start 4-byte aligned: pitch x bytes per sample a multiple of 4 - two 8-bit samples too many, one 16-bit sample too many
        bad("an 8-bit luma pitch of width + 2", b"rows have to start 4-byte aligned", src_pitch_y=world.w + 2)
        bad("an 8-bit chroma pitch of width / 2 + 1", b"rows have to start 4-byte aligned", src_pitch_c=world.w // 2 + 1)
        bad("a 16-bit luma pitch of width + 1", b"rows have to start 4-byte aligned", pic=bare16, P=Pi.ctypes.data, X=None, src_pitch_y=world.w + 1)
        bad("a 16-bit chroma pitch of width / 2 + 3", b"rows have to start 4-byte aligned", pic=bare16, P=Pi.ctypes.data, X=None, src_pitch_c=world.w // 2 + 3)
        bad("no motion field", b"co-located motion field", d_tmvp=None)
        bad("a field at an odd address", b"8-byte aligned", d_tmvp=inp.ptr("tmvp") + 4)
        # the two slot refusals are one text behind this entry and the blocking ones (tests/test_gpu_md.py holds them there): the whole string
        bad("ME records of an empty slot", M.ENTRY.encode() + b": slot 0 does not hold the motion-estimation records of a 416 x 240 picture (none launched for the slot's "
            b"current picture, or only a part of it)", whole=True, d_me=None, me_slot=0)
        bad("OIS records of an empty slot", M.ENTRY.encode() + b": slot 1 does not hold the open-loop intra search records of a 416 x 240 picture", whole=True,
            d_ois=None, ois_slot=1)
        bad("a slot out of range", M.ENTRY.encode() + b": slot -1 does not hold the open-loop intra search records of a 416 x 240 picture", whole=True,
            d_ois=None, ois_slot=-1)
        rect = Rect(0, 0, world.w, world.h)
        ok(lib, lib.svt_amd_encdec_picture_set_rect(world.ctx, world.pic, C.byref(rect)))
        bad("a rank rectangle", b"rank rectangle")
        ok(lib, lib.svt_amd_encdec_picture_set_rect(world.ctx, world.pic, None))
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        assert inp.dev.get()[inp.at["status"]:].tobytes() == bytes([SENTINEL]) * (C.sizeof(M.LaunchStatus) + inp.GUARD)     # nothing was queued
        # DECIDE_ONLY: the blocking P / B call without works and results - the same decisions, and no work records for the consumers
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, flags=M.DECIDE_ONLY), inp))
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        only = M.fetch(lib, world.ctx, world.pic, world.n)
        field = DeviceBuffer(lib, world.ctx, (world.n + 1) * FIELD_REC)
        poc = np.ascontiguousarray(world.X["ref_poc"][0], np.uint64)
        rc = lib.svt_amd_encdec_picture_motion_field(world.ctx, world.pic, 0, poc.ctypes.data, field.ptr, None)
        field.free()
        assert rc == BAD_PARAM and not any(only[1]) and not any(only[2])
        got, _ = launched(lib, world, inp)
        assert decisions(only[0]) == decisions(got[0])
        rc, want = world.call(host=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()
        same_call(want, got, "after the refusals")
        # cost == NULL keeps the rate tables svt_amd_encdec_picture_set_inter put on the object: the same picture, the same bytes
        ok(lib, M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, tiles_of(world.lcus), cost=False), inp))
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        same_call(want, M.fetch(lib, world.ctx, world.pic, world.n), "the object's own rate tables")
    finally:
        lib.svt_amd_encdec_picture_destroy(world.ctx, bare)
        lib.svt_amd_encdec_picture_destroy(world.ctx, bare16)
        inp.free()
        world.free()


# ---- 6. the call does not wait for the picture ------------------------------------------------------------------------------------------------------------------

def test_the_launch_returns_before_the_picture_is_decided(lib):
    """510 LCUs, the longest kernel of the fixtures: blocking call and launch alternate three times in one process, a synchronise behind every launch.  The median
    host time inside the launch call is below half that of the blocking call (the expected ratio is far larger; half is the margin against a noisy host)"""
    g = load("i_motion_1920x1080_m10")
    ctx = make_context(lib, 1920, 1080, 2)
    obj = Obj(lib, ctx, g, 0)
    assert obj.n == 510
    inp = obj.inputs()
    job = M.make_job(obj, inp)
    try:
        ok(lib, lib.svt_amd_md_picture_warmup(ctx, obj.pic))
        blocking, launch = [], []
        for _ in range(3):
            want = obj.blocking()
            blocking.append(obj.seconds)
            t0 = time.perf_counter()
            rc = M.launch(lib, ctx, obj.pic, job, inp)
            launch.append(time.perf_counter() - t0)
            ok(lib, rc)
            ok(lib, lib.svt_amd_synchronize(ctx))
        got = M.fetch(lib, ctx, obj.pic, obj.n)
        same_call(want, got, "1080p")
        mb, ml = sorted(blocking)[1], sorted(launch)[1]
        print("host time inside the call, median of 3: blocking %.3f ms, launch %.3f ms (all: %s / %s)" % (
            1e3 * mb, 1e3 * ml, ["%.3f" % (1e3 * v) for v in blocking], ["%.3f" % (1e3 * v) for v in launch]))
        assert ml < 0.5 * mb, (ml, mb)
    finally:
        inp.free()
        obj.free()
        lib.svt_amd_context_destroy(ctx)
